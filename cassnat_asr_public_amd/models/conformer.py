"""Drop-in for the inference half of the reference's ``models.conformer`` (src/models/conformer.py): the autoregressive (AST)
model with a conformer encoder - what ``ArtTask`` builds for ``model_type: conformer`` and what ``CassNATTask`` loads as the
ESA ranker for ``rank_model: at_baseline`` with a conformer ranker YAML (egs/librispeech/conf/rank_model.yaml).

The encoder is conformer_blocks.Encoder (macaron Swish FFNs at half residual weight, relative-position self attention, the
convolution module; relative positions only, no absolute PE on the source side); the decoder is the transformer decoder with
a Swish feed-forward of width ``d_decff`` (conformer.py:30) at residual weight 1.  On the device this is an engine with
``ast = 1, conf_enc = 1`` (include/cassnat_hip.h): every decode path of ``Transformer`` - ``beam_decode`` (device or host
beam), ``fast_decode_with_ctc``, ``teacher_score`` - runs unchanged on it.
"""
import torch.nn as nn

from .cassnat import _ConformerStack, _ConvEmbedding, _Generator, _Norm, _Stack, create_pe
from .transformer import Transformer, _Lut


class _NormGenerator(_Generator):
    """Generator(add_norm=True) (conformer.py:47-59): the intermediate-CTC head - proj, then norm (not used in decoding)."""

    def __init__(self, d, vocab):
        super().__init__(d, vocab)
        self.norm = _Norm(d)


class Conformer(Transformer):
    """Attribute names are the checkpoint key prefixes of the reference (src/models/conformer.py:34-40 on transformer.py:55-64)."""

    def __init__(self, input_size, args):
        pos_type = getattr(args, "pos_type", "relative")
        if pos_type != "relative":
            raise NotImplementedError("conformer pos_type '%s': the absolute form runs the convolution module before self attention "
                                      "(conformer_blocks.py:32-34), an order the accelerated encoder does not have" % pos_type)
        if getattr(args, "share_ff", False):
            raise NotImplementedError("conformer share_ff: one feed-forward module for both macaron halves is outside the "
                                      "accelerated path")
        nn.Module.__init__(self)
        d, h = args.d_model, args.n_head
        self.src_embed = _ConvEmbedding(input_size, d, args.enc_max_relative_len)
        self.tgt_embed = nn.ModuleList([_Lut(args.vocab_size, d)])  # "tgt_embed.0.lut.weight"
        self.encoder = _ConformerStack(d, h, args.d_encff, args.enc_kernel_size, args.N_enc, False, True)
        self.decoder = _Stack(d, args.d_decff, args.N_dec, True, True, True)
        self.ctc_generator = _Generator(d, args.vocab_size)
        self.att_generator = _Generator(d, args.vocab_size)
        if getattr(args, "interctc_alpha", 0) > 0:
            self.interctc_generator = _NormGenerator(d, args.vocab_size)
        self.pe = create_pe(d)
        self._hyper = dict(input_size=input_size, d_model=d, n_head=h, d_encff=args.d_encff, d_decff=args.d_decff,
                           N_enc=args.N_enc, N_extra=0, N_self_dec=0, N_mix_dec=args.N_dec, vocab_size=args.vocab_size, ast=1,
                           conf_enc=1, enc_max_rel=args.enc_max_relative_len, enc_kernel=args.enc_kernel_size)
        self.hip_precision = getattr(args, "hip_precision", "bf16")
        if self.hip_precision == "fp8":  # (the e4m3 encoder mode is the transformer NAT recogniser's: this model runs bf16 beside it)
            self.hip_precision = "bf16"
        self.hip_max_batch = getattr(args, "hip_max_batch", 32)
        self.hip_max_frames = getattr(args, "hip_max_frames", 2048)
        self._engine = None
        self._engine_key = None


def make_model(input_size, args):
    """Same role as src/models/conformer.py:18-45."""
    model = Conformer(input_size, args)
    for p in model.parameters():  # (the frozen position table stays as it is, as in models/cassnat.py)
        if p.dim() > 1 and p.requires_grad:
            nn.init.xavier_uniform_(p)
    return model
