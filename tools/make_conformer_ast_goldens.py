"""Generates the conformer-AST fixtures tests/golden/conf_ast_*.npz, conf_art_tiny_correct_bw{1,3}.npz and esa_at_conf_tiny.npz
by running the reference's own src/models/conformer.py (the autoregressive model with a conformer encoder).

Runs ONLY on a development machine that holds the reference checkout (oracle.make_goldens.import_reference names its path);
nothing that runs on the GPU machines imports this file.  The weights and features are this package's seeded ones
(cassnat_asr_public_amd.synth), loaded into the reference model through its own state-dict names; the fixtures are data only.

    python tools/make_conformer_ast_goldens.py
"""
import copy
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle.make_goldens import _Vocab, import_reference  # noqa: E402
from cassnat_asr_public_amd import synth  # noqa: E402

GDIR = os.path.join(REPO, "tests", "golden")


def reference_conformer(torch, args, state):
    """The reference's models.conformer.make_model with ``state`` loaded; asserts the parameter names and order."""
    from models.conformer import make_model as make_conf

    model = make_conf(args.input_size, copy.deepcopy(args)).eval()
    named = dict(model.named_parameters())
    shapes = synth.param_shapes_conformer_ast(args)
    assert list(named.keys()) == list(shapes.keys()), "conformer AST parameter naming drifted from the reference"
    assert all(tuple(p.shape) == shapes[k] for k, p in named.items()), "conformer AST parameter shapes drifted from the reference"
    with torch.no_grad():
        for k, p in named.items():
            p.copy_(torch.from_numpy(state[k]))
    return model


def pack(top, W, key="score", fill=-np.inf):
    L = max([len(s["hyp"]) for t in top for s in t] + [1])
    hyp = np.zeros((len(top), W, L), np.int32)
    hlen = np.zeros((len(top), W), np.int32)
    score = np.full((len(top), W), fill)
    n = np.zeros(len(top), np.int32)
    for b, t in enumerate(top):
        n[b] = len(t)
        for j, s in enumerate(t):
            hlen[b, j] = len(s["hyp"])
            hyp[b, j, : hlen[b, j]] = s["hyp"]
            score[b, j] = s[key]
    return hyp, hlen, score, n


def beam_case(torch, name, args, state, feats):
    model = reference_conformer(torch, args, state)
    src = torch.from_numpy(feats)
    with torch.no_grad():
        top = model.beam_decode(src, (src[:, :, 0] != args.padding_idx).unsqueeze(1), _Vocab, copy.deepcopy(args))
    hyp, hlen, score, _ = pack(top, args.beam_width)
    np.savez_compressed(os.path.join(GDIR, name + ".npz"), beam_hyp=hyp, beam_len=hlen, beam_score=score)
    print(name, hlen[:, 0], score[:, 0])


def main():
    torch, make_cassnat = import_reference()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    from utils.beam_decode import ctc_beam_decode

    # joint CTC / attention beam search, tiny shape (gemm path of the engine: d_model 128)
    st = synth.make_state(synth.make_args_ast("tiny_conf_ast"), seed=3, gain=2.0)
    f, _ = synth.make_feats(3, 61, 80, lengths=[61, 57, 51], seed=11)
    for name, ov in {"conf_ast_tiny_att": dict(ctc_weight=0.0), "conf_ast_tiny_ctc": dict(ctc_weight=0.3)}.items():
        beam_case(torch, name, synth.make_args_ast("tiny_conf_ast", beam_width=3, ctc_beam=5, max_decode_ratio=0.5, **ov), st, f)

    # config-4 decoder (d 256, 6 layers, d_decff 2048: the fused Swish kernels, the decode step's d_ff split included) behind a
    # 3-layer conformer encoder of the shipped ranker's shape
    a4 = synth.make_args_ast("config4_conf", N_enc=3, max_decode_ratio=0.3, ctc_weight=0.3)
    st4 = synth.make_state(a4, seed=5)
    f4, _ = synth.make_feats(4, 300, 80, lengths=[300, 287, 262, 231], seed=31)
    beam_case(torch, "conf_ast_c4", a4, st4, f4)

    # ArtTask ctc_correct (fast_decode_with_ctc) and, at bw 1, ctc_only (the CTC prefix beam search of the same model)
    fa, za = synth.make_feats(3, 61, 80, lengths=[61, 57, 51], seed=11)
    for bw in (1, 3):
        aa = synth.make_args_ast("tiny_conf_ast", beam_width=bw, ctc_beam=5, ctc_pruning=8, ctc_lp=0.2, ctc_lm_weight=0,
                                 length_penalty=0.1, use_gpu=False, lm_weight=0)
        model = reference_conformer(torch, aa, st)
        src = torch.from_numpy(fa)
        x_mask = (src[:, :, 0] != 0).unsqueeze(1)
        with torch.no_grad():
            top = model.fast_decode_with_ctc(src, x_mask, _Vocab, copy.deepcopy(aa), None)
        bh, bl, bs, _ = pack(top, bw)
        keep = dict(beam_hyp=bh, beam_len=bl, beam_score=bs)
        if bw == 1:
            with torch.no_grad():
                topc = ctc_beam_decode(model, src, x_mask, torch.from_numpy(za), _Vocab, copy.deepcopy(aa), None)
            ch, cl, cs, cn = pack(topc, aa.ctc_beam, key="score_ctc", fill=-1e10)
            keep.update(ctc_hyp=ch, ctc_len=cl, ctc_score=cs, ctc_n=cn)
        np.savez_compressed(os.path.join(GDIR, f"conf_art_tiny_correct_bw{bw}.npz"), **keep)
        print("conf_art_tiny bw", bw, bl[:, 0], bs[:, 0])

    # ESA (sample_num 4) ranked by the conformer AST (rank_model 'at_baseline'), the select seed of esa_at_tiny
    ae = synth.make_args("tiny", sample_num=4, threshold=0.9, rank_model="at_baseline")
    aa = synth.make_args_ast("tiny_conf_ast")
    se = synth.make_state(ae, seed=0, gain=2.0)
    fe, ze = synth.make_feats(3, 61, 80, lengths=[61, 50, 37], seed=11)
    model = make_cassnat(ae.input_size, ae).eval()
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(torch.from_numpy(se[k]))
    ast = reference_conformer(torch, aa, st)
    src = torch.from_numpy(fe)
    t_sub = ((fe.shape[1] - 1) // 2 + 1 - 1) // 2 + 1
    torch.manual_seed(999)
    select = torch.randint(0, 2, (fe.shape[0] * ae.sample_num, t_sub, 1))
    torch.manual_seed(999)
    with torch.no_grad():
        top, _ = model.beam_decode(src, (src[:, :, 0] != 0).unsqueeze(1), torch.from_numpy(ze), _Vocab, ae, ast)
    U = max(len(t[0]["hyp"]) for t in top)
    hyp = np.zeros((len(top), U), np.int32)
    hlen = np.zeros(len(top), np.int32)
    for b, t in enumerate(top):
        hlen[b] = len(t[0]["hyp"])
        hyp[b, : hlen[b]] = t[0]["hyp"]
    np.savez_compressed(os.path.join(GDIR, "esa_at_conf_tiny.npz"), hyp=hyp, hyp_len=hlen, select=select.numpy().astype(np.uint8),
                        score=np.array([t[0]["score"] for t in top], np.float64))
    print("esa_at_conf_tiny", hlen, [t[0]["score"] for t in top])


if __name__ == "__main__":
    main()
