"""Generates the CASS-NAT + LM fixtures, tests/golden/nat_lm_*.npz, by running the reference's own CassNAT.beam_decode
(src/models/cassnat.py:420-637) with ``args.lm_weight > 0`` and its own TransformerLM (src/models/lm.py) as ``lm_model``.

Runs ONLY on a development machine that holds the reference checkout (oracle.make_goldens.import_reference names its path);
nothing that runs on the GPU machines imports this file.  The weights and features are this package's seeded ones
(cassnat_asr_public_amd.synth), loaded into the reference models through their own state-dict names; the fixtures are data only:
beam_hyp / beam_len / beam_score, the row counts the finish loop read (ylen), the ESA draws (select) and, for the tiny cases
without ESA, the reference's att_out.

    python tools/make_nat_lm_goldens.py [name ...]
"""
import copy
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from oracle.make_goldens import _Vocab, import_reference  # noqa: E402
from nat_lm_cases import CASES, WITH_ATT_OUT  # noqa: E402

GDIR = os.path.join(REPO, "tests", "golden")


def load(model, state, torch):
    named = dict(model.named_parameters())
    assert list(named.keys()) == list(state.keys()), "parameter naming drifted from the reference"
    with torch.no_grad():
        for k, p in named.items():
            assert tuple(p.shape) == state[k].shape, k
            p.copy_(torch.from_numpy(state[k]))
    return model.eval()


def pack(top, W):
    L = max(len(s["hyp"]) for t in top for s in t)
    hyp = np.zeros((len(top), W, L), np.int32)
    hlen = np.zeros((len(top), W), np.int32)
    score = np.full((len(top), W), -np.inf)
    for b, t in enumerate(top):
        assert len(t) == W
        for j, s in enumerate(t):
            hlen[b, j] = len(s["hyp"])
            hyp[b, j, : hlen[b, j]] = s["hyp"]
            score[b, j] = s["score"]
            # (the reference grows ys with the hypothesis when the LM is on)
            assert tuple(s["ys"].shape) == (1, len(s["hyp"])) and s["ys"][0].tolist() == s["hyp"]
    return hyp, hlen, score


def key_gaps(hyp_len, score, lp):
    """Smallest gap between the sort keys of neighbouring final beams, per utterance."""
    key = score + (hyp_len - 1) * (lp if lp is not None else 0.0)
    return [float(np.min(-np.diff(key[b]))) if key.shape[1] > 1 else float("inf") for b in range(key.shape[0])]


def case(torch, make_model, name):
    from models.lm import make_model as make_lm
    from utils.beam_decode import ctc_beam_decode

    args, state, feats, sizes, lm_args, lm_state, extra = CASES[name]()
    model = load(make_model(args.input_size, copy.deepcopy(args)), state, torch)
    lm = load(make_lm(copy.deepcopy(lm_args)), lm_state, torch)
    cap = {}
    hook = model.att_generator.register_forward_hook(lambda m_, i_, o_: cap.__setitem__("att_out", o_.detach().clone()))
    orig_a2m, orig_bpa, orig_vit = model.align_to_mask, model.best_path_align, model.viterbi_align

    def a2m(*p, **k):
        r = orig_a2m(*p, **k)
        cap["ylen"] = r[1].clone()
        return r

    def bpa(*p, **k):
        r = orig_bpa(*p, **k)
        cap.setdefault("ylen", r[1].clone())  # (use_trigger False: the loop reads best_path_align's own counts)
        return r

    def vit(*p, **k):
        # As shipped, beam_path_align passes a stray 8th positional argument to the 7-parameter viterbi_align (cassnat.py:413 vs
        # :272), so decode_type 'ctc_att' raises TypeError in the unmodified reference.  This harness-side wrapper drops it
        # (reference files untouched), as oracle/make_goldens.py does for ctcbeam_tiny.
        return orig_vit(*p[:7], **k)

    model.align_to_mask, model.viterbi_align = a2m, vit
    if not args.use_trigger:
        model.best_path_align = bpa
    src = torch.from_numpy(feats)
    x_mask = (src[:, :, 0] != args.padding_idx).unsqueeze(1)
    keep = {}
    top_ctc = None
    t0 = time.time()
    with torch.no_grad():
        if extra.get("ctc_att"):
            top_ctc = ctc_beam_decode(model, src, x_mask, torch.from_numpy(sizes), _Vocab, copy.deepcopy(args), None)
        if "select_seed" in extra:
            t_sub = ((feats.shape[1] - 1) // 2 + 1 - 1) // 2 + 1
            torch.manual_seed(extra["select_seed"])
            keep["select"] = torch.randint(0, 2, (feats.shape[0] * args.sample_num, t_sub, 1)).numpy().astype(np.uint8)
            torch.manual_seed(extra["select_seed"])
        top, _ = model.beam_decode(src, x_mask, torch.from_numpy(sizes), _Vocab, copy.deepcopy(args), lm, top_ctc)
    hook.remove()
    hyp, hlen, score = pack(top, args.beam_width)
    if extra.get("needs_blank"):  # the LM key mask must see a blank inside some kept prefix
        assert any(0 in s["hyp"][:-1] for t in top for s in t), "no kept beam holds token 0 inside its prefix: pick another seed"
    ylen = cap["ylen"].numpy().astype(np.int32).reshape(feats.shape[0], -1)  # (B, sample_num) with ESA, else (B,)
    if args.sample_num <= 1:
        ylen = ylen[:, 0]
    keep.update(beam_hyp=hyp, beam_len=hlen, beam_score=score, ylen=ylen)
    if name in WITH_ATT_OUT:
        keep["att_out"] = cap["att_out"].numpy().astype(np.float32)
    path = os.path.join(GDIR, name + ".npz")
    np.savez_compressed(path, **keep)
    assert os.path.getsize(path) < 100 * 1024, path
    print(name, "%.1fs" % (time.time() - t0), "len", hlen[:, 0].tolist(), "score", score[:, 0].tolist(), "key gaps",
          key_gaps(hlen, score, args.length_penalty), "%d bytes" % os.path.getsize(path))


def main():
    torch, make_model = import_reference()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    for name in sys.argv[1:] or list(CASES):
        case(torch, make_model, name)


if __name__ == "__main__":
    main()
