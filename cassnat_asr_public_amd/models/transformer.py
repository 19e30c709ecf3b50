"""Drop-in for the inference half of the reference's ``models.transformer`` (src/models/transformer.py): the
autoregressive (AST) model with joint CTC/attention beam search - BASELINE config 4, SURVEY 8a row a18.

Same surface: ``make_model(input_size, args) -> Transformer`` with the reference's parameter names, and
``Transformer.beam_decode(src, src_mask, vocab, args, lm_model=None) -> batch_top_seqs``.  By default the WHOLE search
runs on the device (``cn_decode_ast``): token embedding, the decoder layers on the NEW position only (keys/values of
the prefix come from a KV cache addressed through per-hypothesis ancestor tables; the reference re-runs the decoder
on the whole prefix), generator + log-softmax + top-k, the CTC prefix scorer and the beam bookkeeping
(transformer.py:157-240) - no host round trip per step.  ``args.hip_host_beam = True`` keeps the bookkeeping in
Python over ``cn_ast_begin / cn_ast_step / cn_ast_ctc_score`` (same results; used to cross-check the device beam).
With ``args.lm_weight > 0`` the TransformerLM ``lm_model`` (models.lm) is fused (transformer.py:186-209): its incremental
step runs beside the decoder's on the same ancestor / key-mask tables (``cn_ast_attach_lm``, ``cn_ast_step_lm``).
"""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

from .. import hip
from .cassnat import _ConvEmbedding, _Generator, _Params, _Stack, create_pe


class _Lut(_Params):
    def __init__(self, vocab, d):
        super().__init__()
        self.lut = nn.Embedding(vocab, d)


class Transformer(nn.Module):
    """Attribute names are the checkpoint key prefixes of the reference (src/models/transformer.py:55-60)."""

    def __init__(self, input_size, args):
        super().__init__()
        d = args.d_model
        self.src_embed = _ConvEmbedding(input_size, d)
        self.tgt_embed = nn.ModuleList([_Lut(args.vocab_size, d)])  # "tgt_embed.0.lut.weight"
        self.encoder = _Stack(d, args.d_ff, args.N_enc, True, False, True)
        self.decoder = _Stack(d, args.d_ff, args.N_dec, True, True, True)
        self.ctc_generator = _Generator(d, args.vocab_size)
        self.att_generator = _Generator(d, args.vocab_size)
        self.pe = create_pe(d)
        self._hyper = dict(input_size=input_size, d_model=d, n_head=args.n_head, d_encff=args.d_ff, d_decff=args.d_ff,
                           N_enc=args.N_enc, N_extra=0, N_self_dec=0, N_mix_dec=args.N_dec, vocab_size=args.vocab_size, ast=1)
        self.hip_precision = getattr(args, "hip_precision", "bf16")
        if self.hip_precision == "fp8":  # the e4m3 products are the NAT recogniser's encoder (BASELINE config 5): this model runs bf16 beside it
            self.hip_precision = "bf16"
        self.hip_max_batch = getattr(args, "hip_max_batch", 32)
        self.hip_max_frames = getattr(args, "hip_max_frames", 2048)
        self._engine = None
        self._engine_key = None

    def cuda(self, device=None):
        self._device = 0 if device is None else (device if isinstance(device, int) else torch.device(device).index or 0)
        return self

    def forward(self, *a, **k):
        raise NotImplementedError("training forward is out of scope; use beam_decode")

    def _new_handle(self, batch, frames, share_with=None, esa_group=1):
        return hip.Engine(SimpleNamespace(**self._hyper), precision=self.hip_precision,
                          max_batch=max(batch, self.hip_max_batch), max_frames=max(frames, self.hip_max_frames),
                          device=getattr(self, "_device", torch.cuda.current_device()), share_with=share_with, esa_group=esa_group)

    def teacher_score(self, feats, lm_input, target, length, n_per_utt, U, args):
        """ESA ranking with ``rank_model == 'at_baseline'`` (src/models/cassnat.py:514-520): this model's encoder on the B
        utterances, then its decoder teacher-forced on ``lm_input`` (N = B * n_per_utt rows, row e of utterance e % B) ->
        log-probabilities of ``target`` (float32 (N, ld) cuda; the reference takes softmax probabilities: ``.exp()``)."""
        B, T, _ = feats.shape
        eng = self._engine
        key = (tuple(p._version for p in self.parameters()), self.hip_precision)
        if (eng is None or self._engine_key != key or B > eng.cfg.max_batch or T > eng.cfg.max_frames
                or n_per_utt > max(1, eng.cfg.esa_group)):
            if eng is not None and self._engine_key == key:
                new = self._new_handle(B, T, share_with=eng, esa_group=n_per_utt)
                eng.close()
            else:
                if eng is not None:
                    eng.close()
                new = self._new_handle(B, T, esa_group=n_per_utt)
                new.load_state({k: v.detach() for k, v in self.named_parameters()}, self.pe)
            self._engine, self._engine_key = new, key
            eng = new
        opts = hip.CnDecodeOpts(padding_idx=int(args.padding_idx), sos=1, beam_width=1)
        score = torch.zeros(lm_input.shape, dtype=torch.float32, device=lm_input.device)
        eng.ast_teacher_score(feats, opts, lm_input, target, length, n_per_utt, U, score)
        return score

    def build_engine(self, batch, frames, with_weights=True):
        """The model's engine.  Current weights are never re-packed: a rebuild for a larger workspace shares the old handle's
        device blob.  ``with_weights=False``: layout only, the blob arrives by RCCL broadcast (dist.broadcast_weights)."""
        key = (tuple(p._version for p in self.parameters()), self.hip_precision)
        old = self._engine
        if old is not None and self._engine_key == key and old.finalized:
            eng = self._new_handle(batch, frames, share_with=old)
            old.close()
        else:
            if old is not None:
                old.close()
            if with_weights and getattr(self, "_remote_version", None) == key[0]:
                raise hip.HipError("this rank's parameters were never loaded (its weights arrived by broadcast)")
            eng = self._new_handle(batch, frames)
            if with_weights:
                eng.load_state({k: v.detach() for k, v in self.named_parameters()}, self.pe)
            else:
                eng.finalize()
                self._remote_version = key[0]
        self._engine, self._engine_key = eng, key
        return eng

    def new_engine(self, batch, frames, share):
        """A further handle (own workspace and KV cache) on the device blob of ``share``: what a decode pipeline owns."""
        return self._new_handle(batch, frames, share_with=share)

    def engine(self, batch, frames):
        key = (tuple(p._version for p in self.parameters()), self.hip_precision)
        if (self._engine is None or self._engine_key != key or batch > self._engine.cfg.max_batch
                or frames > self._engine.cfg.max_frames):
            self.build_engine(batch, frames)
        return self._engine

    def beam_decode(self, src, src_mask, vocab, args, lm_model=None, engine=None, lm_engine=None, bias=None):
        """Same contract as the reference's Transformer.beam_decode (src/models/transformer.py:122-241), LM shallow fusion
        included (``args.lm_weight > 0`` with ``lm_model`` a models.lm.TransformerLM).  ``engine``: run on this handle (a decode
        pipeline's, see ``new_engine``) instead of the model's own; ``lm_engine``: the pipeline's LM handle
        (TransformerLM.new_engine) instead of the LM's own.

        ``lm_model`` a models.ngram.NgramLM (``rank_model: n-gram`` with an ARPA file): word n-gram shallow fusion
        (include/cassnat_hip_ast_ngram.h) - the model's device tables are attached with float32(lm_weight * ln 10) for the call.
        The ``hip_host_beam`` loop takes its per-hypothesis adds from ``lm_model.ast_adds_host``; any object that offers that
        method beside ``desc`` / ``cuda`` / ``device_ok`` serves there.

        ``bias`` a models.bias.BiasList (the keyword, else ``args.hip_bias_model`` when ``args.hip_bias_search == "att"``):
        contextual phrase biasing (include/cassnat_hip_ast_bias.h) - the list's device tables are attached for the call.  The
        ``hip_host_beam`` loop takes the hypotheses' nodes from ``bias.ast_nodes_host`` and, with CTC, the terms of its update from
        ``bias.ast_terms_host``; any object that offers those two methods beside ``desc`` / ``cuda`` serves there.  A list together
        with a fused language model is refused."""
        lm_weight = float(getattr(args, "lm_weight", 0) or 0)
        if bias is None and getattr(args, "hip_bias_search", "ctc") == "att":
            bias = getattr(args, "hip_bias_model", None)
        if bias is not None and lm_weight > 0:
            raise NotImplementedError("--hip_bias (hip_bias_search att) together with a language model fused into the AST beam search "
                                      "(lm_weight > 0) is not on the accelerated path: drop one of the two")
        if lm_weight <= 0:
            return self._beam_decode(src, args, vocab, engine, None, 0.0, bias=bias)
        if lm_model is None:
            raise ValueError("beam_decode: lm_weight > 0 needs lm_model")
        if hasattr(lm_model, "ast_adds_host"):
            if not lm_model.device_ok:
                raise ValueError("a piece of the vocabulary has a separator behind its leading run: its hypotheses cannot be glued into "
                                 "words, so the AST beam search cannot fuse the n-gram model")
            # (ARPA scores are log10, the attention and CTC scores natural logarithms)
            return self._beam_decode(src, args, vocab, engine, None, 0.0, ngram=lm_model, ngram_scale=float(np.float32(lm_weight * math.log(10.0))))
        bw = int(args.beam_width)
        B = src.shape[0]
        lm_eng = lm_engine if lm_engine is not None else lm_model.step_engine(B * bw)
        return self._beam_decode(src, args, vocab, engine, lm_eng, lm_weight)

    def _beam_decode(self, src, args, vocab, engine, lm_eng, lm_weight, ngram=None, ngram_scale=0.0, bias=None):
        sos, eos = vocab.word2index["sos"], vocab.word2index["eos"]
        assert vocab.word2index["blank"] == args.padding_idx
        dev = torch.device("cuda", getattr(self, "_device", torch.cuda.current_device()))
        feats = src.to(dev, torch.float32).contiguous()
        B, T, _ = feats.shape
        Tp = hip.subsampled(T)
        eng = engine if engine is not None else self.engine(B, T)
        use_ctc = args.ctc_weight > 0
        bw = int(args.beam_width)
        K = int(args.ctc_beam) if use_ctc else bw
        max_step = int(args.max_decode_ratio * Tp) if args.max_decode_ratio > 0 else Tp
        max_len = max_step + 1
        opts = hip.CnDecodeOpts(padding_idx=int(args.padding_idx), sos=sos, beam_width=1)
        eng.ast_attach_lm(lm_eng)  # (None detaches: a handle never keeps an LM from an earlier call)
        eng.ast_attach_ngram(None)
        eng.ast_attach_bias(None)
        try:
            if ngram is not None:
                ngram.cuda(dev)
                eng.ast_attach_ngram(ngram.desc(dev), ngram_scale)
            if bias is not None:
                bias.cuda(dev)
                eng.ast_attach_bias(bias.desc(dev))
            return self._beam_search(eng, feats, opts, args, sos, eos, bw, K, use_ctc, max_step, lm_weight, dev, ngram, ngram_scale, bias)
        finally:
            if lm_eng is not None:
                eng.ast_attach_lm(None)
            if ngram is not None:
                eng.ast_attach_ngram(None)
            if bias is not None:
                eng.ast_attach_bias(None)

    def _beam_search(self, eng, feats, opts, args, sos, eos, bw, K, use_ctc, max_step, lm_weight, dev, ngram=None, ngram_scale=0.0, bias=None):
        B = feats.shape[0]
        max_len = max_step + 1
        use_lm = lm_weight > 0
        lp = args.length_penalty
        if not getattr(args, "hip_host_beam", False):
            ao = hip.CnAstOpts(ctc_weight=float(args.ctc_weight) if use_ctc else 0.0, temperature=float(args.T), ctc_beam=K,
                               beam_width=bw, max_step=max_step, eos=eos, use_length_penalty=int(lp is not None),
                               one_minus_ctc_weight=float(1 - args.ctc_weight),
                               length_penalty=float(lp) if lp is not None else 0.0, lm_weight=lm_weight)
            hyp = torch.empty(B, bw, max_len, dtype=torch.int32, device=dev)
            hlen = torch.empty(B, bw, dtype=torch.int32, device=dev)
            score = torch.empty(B, bw, dtype=torch.float64, device=dev)
            eng.ast_decode(feats, opts, ao, hyp, hlen, score)
            hyp, hlen, score = hyp.cpu().numpy(), hlen.cpu().numpy(), score.cpu().numpy()
            eng.check_range("Transformer.beam_decode")  # (fp16 engines: the features were inside the half-precision range)
            out = []
            for b in range(B):
                row = []
                for j in range(bw):
                    h = hyp[b, j, : hlen[b, j]].tolist()
                    row.append({"ys": torch.tensor([h], dtype=torch.long), "score": float(score[b, j]), "hyp": h})
                out.append(row)
            return out
        eng.ast_begin(feats, opts, use_ctc, max_len, B * bw, K if use_ctc else 0)
        w32 = np.float32(args.ctc_weight)
        u32 = np.float32(1 - args.ctc_weight)
        lw32 = np.float32(1.0 if bias is not None else (ngram_scale if ngram is not None else lm_weight))

        beams = [[{"score": 0.0, "hyp": [sos], "anc": [], "ctc_ref": -1 - b, "ctc_prev": np.float32(0.0)}] for b in range(B)]
        idx_d = torch.empty(B * bw, K, dtype=torch.int32, device=dev)
        val_d = torch.empty(B * bw, K, dtype=torch.float32, device=dev)
        ctc_d = torch.empty(B * bw, K, dtype=torch.float32, device=dev)
        lm_d = torch.empty(B * bw, K, dtype=torch.float32, device=dev)
        for i in range(max_step):
            live = [(b, s) for b in range(B) for s in beams[b] if s["hyp"][-1] != eos]
            if not live:
                break
            n = len(live)
            tok = np.array([s["hyp"][-1] for _, s in live], np.int32)
            utt = np.array([b for b, _ in live], np.int32)
            anc = np.zeros((n, max_len), np.int32)
            keyok = np.zeros((n, max_len), np.uint8)
            for k, (_, s) in enumerate(live):
                anc[k, :i] = s["anc"]
                anc[k, i] = k
                keyok[k, : i + 1] = [t != args.padding_idx for t in s["hyp"]]
            tok_d, utt_d = torch.from_numpy(tok).to(dev), torch.from_numpy(utt).to(dev)
            anc_d, keyok_d = torch.from_numpy(anc).to(dev), torch.from_numpy(keyok).to(dev)
            if ngram is not None:  # as use_lm, the LM row being the n-gram terms of the hypotheses' own tokens (behind sos)
                rows = np.zeros((n, max(1, i)), np.int32)
                for k, (_, s) in enumerate(live):
                    rows[k, :i] = s["hyp"][1:]
                adds = np.ascontiguousarray(ngram.ast_adds_host(rows, np.full(n, i, np.int32), eos), np.float32).reshape(n, 2)
                eng.ast_step_ngram(i, tok_d, utt_d, anc_d, keyok_d, args.T, K, use_ctc, eos, torch.from_numpy(adds).to(dev), idx_d[:n],
                                   val_d[:n], lm_d[:n])
            elif bias is not None:  # as use_lm, the LM row being the phrase terms for the hypotheses' nodes, the weight 1
                rows = np.zeros((n, max(1, i)), np.int32)
                for k, (_, s) in enumerate(live):
                    rows[k, :i] = s["hyp"][1:]
                nodes = np.ascontiguousarray(bias.ast_nodes_host(rows, np.full(n, i, np.int32)), np.int32).reshape(n)
                eng.ast_step_bias(i, tok_d, utt_d, anc_d, keyok_d, args.T, K, use_ctc, eos, torch.from_numpy(nodes).to(dev), idx_d[:n],
                                  val_d[:n], lm_d[:n])
            elif use_lm:  # no CTC: val = top-K of att + lm_weight * lm; with CTC: attention top-K and the LM at those candidates
                eng.ast_step_lm(i, tok_d, utt_d, anc_d, keyok_d, args.T, K, lm_weight, use_ctc, idx_d[:n], val_d[:n], lm_d[:n])
            else:
                eng.ast_step(i, tok_d, utt_d, anc_d, keyok_d, args.T, K, idx_d[:n], val_d[:n])
            if use_ctc:
                ref_d = torch.from_numpy(np.array([s["ctc_ref"] for _, s in live], np.int32)).to(dev)
                eng.ast_ctc_score(i, utt_d, tok_d, idx_d[:n], ref_d, i & 1, eos, ctc_d[:n])
                ctc = ctc_d[:n].cpu().numpy()
            indices, att = idx_d[:n].cpu().numpy(), val_d[:n].cpu().numpy()
            if use_ctc:
                prev = np.array([s["ctc_prev"] for _, s in live], np.float32)[:, None]
                local = w32 * (ctc - prev) + u32 * att  # float32, same op order as transformer.py:205-206
                if bias is not None:  # (the terms of this update are the host's, not the device's)
                    local = local + lw32 * np.ascontiguousarray(bias.ast_terms_host(nodes, indices, eos), np.float32).reshape(n, K)
                elif use_lm or ngram is not None:
                    local = local + lw32 * lm_d[:n].cpu().numpy()  # transformer.py:208-209
                local_idx = np.argsort(-local, axis=1, kind="stable")[:, :bw]
                local_scores = np.take_along_axis(local, local_idx, 1)
                tokens = np.take_along_axis(indices, local_idx, 1)
            else:
                local_scores, tokens = att[:, :bw], indices[:, :bw]
            cand = [[s for s in beams[b] if s["hyp"][-1] == eos] for b in range(B)]
            for k, (b, s) in enumerate(live):
                for j in range(bw):
                    new = {"score": s["score"] + float(local_scores[k, j]), "hyp": s["hyp"] + [int(tokens[k, j])],
                           "anc": s["anc"] + [k]}
                    if use_ctc:
                        ti = int(local_idx[k, j])
                        new["ctc_ref"] = k * K + ti
                        new["ctc_prev"] = ctc[k, ti]
                    cand[b].append(new)
            for b in range(B):
                if lp is not None:
                    cand[b].sort(key=lambda x: x["score"] + (len(x["hyp"]) - 1) * lp, reverse=True)
                else:
                    cand[b].sort(key=lambda x: x["score"], reverse=True)
                beams[b] = cand[b][:bw]
        eng.check_range("Transformer.beam_decode")
        return [[{"ys": torch.tensor([s["hyp"]], dtype=torch.long), "score": s["score"], "hyp": s["hyp"]} for s in beams[b]]
                for b in range(B)]

    def fast_decode_with_ctc(self, src, src_mask, vocab, args, lm_model=None, engine=None):
        """Same contract as the reference's Transformer.fast_decode_with_ctc (src/models/transformer.py:243-342; ArtTask decode_type
        'ctc_correct'), lm_weight == 0: the CTC greedy hypothesis is the decoder's teacher-forced input, the decoder a correction
        model.  Encoder, CTC collapse, decoder and the per-row top-k run on the device (``cn_ast_ctc_correct``); the finish loop -
        O(rows * beam^2) numbers - is the reference's, here on the host: row i is consumed while i <= length[b], an eos is scored
        but not appended."""
        if getattr(args, "lm_weight", 0) > 0 or lm_model is not None:
            raise NotImplementedError("LM fusion is outside the accelerated path")
        sos, eos = vocab.word2index["sos"], vocab.word2index["eos"]
        assert vocab.word2index["blank"] == args.padding_idx
        dev = torch.device("cuda", getattr(self, "_device", torch.cuda.current_device()))
        feats = src.to(dev, torch.float32).contiguous()
        B, T, _ = feats.shape
        eng = engine if engine is not None else self.engine(B, T)
        bw = int(args.beam_width)
        opts = hip.CnDecodeOpts(padding_idx=int(args.padding_idx), sos=sos, beam_width=1)
        length, tok, val = eng.ast_ctc_correct(feats, opts, bw)
        length, tok, val = length.cpu().numpy(), tok.cpu().numpy(), val.cpu().numpy()
        eng.check_range("Transformer.fast_decode_with_ctc")
        lp = args.length_penalty
        ys = torch.ones(1, 1).fill_(sos).long()
        out = []
        for b in range(B):
            beams = [{"ys": ys, "score": 0.0, "hyp": [sos]}]
            for i in range(int(length[b]) + 1):
                cand = [{"ys": ys, "score": s["score"] + float(val[b, i, j]),
                         "hyp": s["hyp"] + [int(tok[b, i, j])] if int(tok[b, i, j]) != eos else s["hyp"]}
                        for s in beams for j in range(bw)]
                if lp is not None:
                    cand.sort(key=lambda s: s["score"] + (len(s["hyp"]) - 1) * lp, reverse=True)
                else:
                    cand.sort(key=lambda s: s["score"], reverse=True)
                beams = cand[:bw]
            out.append(beams)
        return out


def make_model(input_size, args):
    """Same role as src/models/transformer.py:19-37."""
    model = Transformer(input_size, args)
    for p in model.parameters():
        if p.dim() > 1:
            nn.init.xavier_uniform_(p)
    return model
