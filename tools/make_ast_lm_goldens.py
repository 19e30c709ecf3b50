"""Generates the LM-fusion fixtures of the AST beam search, tests/golden/ast_lm_*.npz, ast_wide_c4.npz and conf_ast_lm_recipe.npz,
by running the reference's own Transformer.beam_decode (src/models/transformer.py:122-241; Conformer inherits it) with its own
TransformerLM (src/models/lm.py) as ``lm_model``.

Runs ONLY on a development machine that holds the reference checkout (oracle.make_goldens.import_reference names its path);
nothing that runs on the GPU machines imports this file.  The weights and features are this package's seeded ones
(cassnat_asr_public_amd.synth), loaded into the reference models through their own state-dict names; the fixtures are data only.

    python tools/make_ast_lm_goldens.py [name ...]
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
from cassnat_asr_public_amd import synth  # noqa: E402
from ast_lm_cases import CASES, lm_step_prefixes  # noqa: E402

GDIR = os.path.join(REPO, "tests", "golden")


def load(model, state, torch):
    named = dict(model.named_parameters())
    assert list(named.keys()) == list(state.keys()), "parameter naming drifted from the reference"
    with torch.no_grad():
        for k, p in named.items():
            assert tuple(p.shape) == state[k].shape, k
            p.copy_(torch.from_numpy(state[k]))
    return model.eval()


def reference_lm(torch, lm_args, lm_state):
    from models.lm import make_model as make_lm

    return load(make_lm(copy.deepcopy(lm_args)), lm_state, torch)


def reference_ast(torch, args, state):
    if getattr(args, "model_type", "transformer") == "conformer":
        from models.conformer import make_model as make_ast
    else:
        from models.transformer import make_model as make_ast
    return load(make_ast(args.input_size, copy.deepcopy(args)), state, torch)


def pack(top, W):
    L = max(len(s["hyp"]) for t in top for s in t)
    hyp = np.zeros((len(top), W, L), np.int32)
    hlen = np.zeros((len(top), W), np.int32)
    score = np.full((len(top), W), -np.inf)
    for b, t in enumerate(top):
        for j, s in enumerate(t):
            hlen[b, j] = len(s["hyp"])
            hyp[b, j, : hlen[b, j]] = s["hyp"]
            score[b, j] = s["score"]
    return hyp, hlen, score


def lm_step_case(torch):
    """ast_lm_step_tiny: lm_model(ys, tgt_mask)[:, -1] for every prefix length of a batch of token rows (some hold token 0),
    under the beam search's mask (ys != padding_idx) & subsequent_mask."""
    _, _, _, lm_args, lm_state, _ = CASES["ast_lm_tiny_att"]()
    lm = reference_lm(torch, lm_args, lm_state)
    ys = lm_step_prefixes()
    n, L = ys.shape
    out = np.zeros((n, L, lm_args.vocab_size), np.float32)
    with torch.no_grad():
        for p in range(L):
            y = torch.from_numpy(ys[:, : p + 1]).long()
            mask = (y != 0).unsqueeze(1) & torch.tril(torch.ones(p + 1, p + 1, dtype=torch.uint8)).unsqueeze(0).bool()
            out[:, p] = lm(y, mask)[:, -1].numpy()
    np.savez_compressed(os.path.join(GDIR, "ast_lm_step_tiny.npz"), ys=ys, lm_logp=out)
    print("ast_lm_step_tiny", ys.shape)


def beam_case(torch, name):
    args, state, feats, lm_args, lm_state, _ = CASES[name]()
    model = reference_ast(torch, args, state)
    lm = reference_lm(torch, lm_args, lm_state) if lm_args is not None else None
    src = torch.from_numpy(feats)
    t0 = time.time()
    with torch.no_grad():
        top = model.beam_decode(src, (src[:, :, 0] != args.padding_idx).unsqueeze(1), _Vocab, copy.deepcopy(args), lm)
    hyp, hlen, score = pack(top, args.beam_width)
    if name == "ast_lm_tiny_att":  # the LM key mask must see a blank in some prefix
        assert any(0 in s["hyp"] for t in top for s in t), "no beam of the att case holds token 0: pick another seed"
    np.savez_compressed(os.path.join(GDIR, name + ".npz"), beam_hyp=hyp, beam_len=hlen, beam_score=score)
    print(name, "%.1fs" % (time.time() - t0), hlen[:, 0], score[:, 0])


def main():
    torch, _ = import_reference()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    names = sys.argv[1:] or ["ast_lm_step_tiny"] + list(CASES)
    for name in names:
        if name == "ast_lm_step_tiny":
            lm_step_case(torch)
        else:
            beam_case(torch, name)


if __name__ == "__main__":
    main()
