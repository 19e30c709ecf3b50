"""ctypes binding of libcassnat_hip.so (the C ABI declared in include/cassnat_hip.h and its companions, abi.py lists them).

The product path has no CPU fallback: if the library is missing or a call fails, this raises.
"""
import ctypes as C
import os

import numpy as np

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# (CASSNAT_HIP_LIB: another build of the same library - A/B measurements of kernel variants, tools/scripts/ab_bench.sh)
LIB_PATH = os.environ.get("CASSNAT_HIP_LIB") or os.path.join(_HERE, "libcassnat_hip.so")
# the second build of the same sources (csrc/common.h: -DCN_OP16_F16): the fast engine with IEEE half-precision MFMA operands -
# --hip_precision fp16.  Same C ABI; an engine keeps the library it was created in.
LIB_PATH_F16 = os.path.join(_HERE, "libcassnat_hip_f16.so")
HEADER_PATH = abi.HEADER_PATH

# the header's enums and #defines under the names the options use
_K = abi.CONSTANTS
_F32, _BF16, _FP8, _BF16X3, _F16 = (_K["CN_PRECISION_" + n] for n in ("F32", "BF16", "FP8", "BF16X3", "F16"))
PRECISION = {"fp32": _F32, "f32": _F32, "float32": _F32, "bf16": _BF16, "bfloat16": _BF16, "fp8": _FP8, "bf16x3": _BF16X3, "fp16": _F16,
             "float16": _F16}
DTYPES = {_K["CN_DTYPE_F32"]: np.float32, _K["CN_DTYPE_I32"]: np.int32, _K["CN_DTYPE_U8"]: np.uint8, _K["CN_DTYPE_F64"]: np.float64}
FP8_SCOPE_BITS = {"conv2": _K["CN_FP8_CONV2"], "linear": _K["CN_FP8_LINEAR"], "ffn": _K["CN_FP8_FFN"]}


def parse_fp8_scope(text):
    """``--hip_fp8_scope``: which encoder-side products of the fp8 engine take e4m3 operands - "all" or a "+"-joined list
    of ``conv2``, ``linear`` (needs conv2) and ``ffn`` / ``ffn:N`` (the feed-forward products of the encoder layers >= N).
    Returns (cn_config.fp8_scope, cn_config.fp8_ffn_first_layer)."""
    text = (text or "all").strip().lower()
    if text == "all":
        return 0, 0
    scope, first = 0, 0
    for part in text.split("+"):
        name, _, arg = part.strip().partition(":")
        if name not in FP8_SCOPE_BITS or (arg and name != "ffn"):
            raise ValueError(f"hip_fp8_scope: unknown part {part!r} (all, or conv2 / linear / ffn[:first layer] joined by +)")
        scope |= FP8_SCOPE_BITS[name]
        if arg:
            first = int(arg)
            if first < 0:
                raise ValueError("hip_fp8_scope: ffn:N needs N >= 0")
    if scope & 2 and not scope & 1:
        raise ValueError("hip_fp8_scope: linear needs conv2 (conv2 hands its rows to linear_out in e4m3)")
    return scope, first


# the ten structs of the header, derived from it field for field (abi.py)
CnConfig, CnDecodeOpts, CnAstOpts, CnFbankOpts, CnAttnDesc, CnNgramDesc, CnChainDesc, CnFrontendDesc, CnGemmDesc, CnProjX3Desc = (abi.STRUCTS[n] for n in (
    "cn_config", "cn_decode_opts", "cn_ast_opts", "cn_fbank_opts", "cn_attn_desc", "cn_ngram_desc", "cn_chain_desc", "cn_frontend_desc", "cn_gemm_desc",
    "cn_proj_x3_desc"))
# the descriptor of the phrase-biasing automaton (include/cassnat_hip_ctc_bias.h declares it beside its entry points)
CnBiasDesc = abi.CTC_BIAS_STRUCTS["cn_bias_desc"]
# the descriptor of the alignment kernel's forms (include/cassnat_hip_align.h declares it beside the entry points of its family)
CnAlignDesc = abi.ALIGN_STRUCTS["cn_align_desc"]
# the descriptor of the fused generator tail's forms (include/cassnat_hip_genmax.h)
CnGenmaxDesc = abi.GENMAX_STRUCTS["cn_genmax_desc"]


class HipError(RuntimeError):
    pass


_libs = {}


def declared_symbols():
    """Every function name include/cassnat_hip.h declares."""
    return sorted(abi.FUNCTIONS)


def lib_for(precision):
    """The library that holds engines of ``precision`` (a name of ``PRECISION`` or its number)."""
    code = PRECISION[precision] if isinstance(precision, str) else int(precision)
    return lib("f16" if code == PRECISION["fp16"] else None)


def lib(flavour=None):
    """Load the shared library (built by __graft_entry__.build / cassnat_asr_public_amd.build).  ``flavour`` "f16": the build with
    half-precision operands (libcassnat_hip_f16.so) - everything that is not an fp16 engine uses the default library."""
    path = LIB_PATH_F16 if flavour == "f16" else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise HipError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(there is no CPU fallback for the CASS-NAT hot path)")
    L = C.CDLL(path)
    abi.bind(L)  # argtypes / restype of every declared function; AttributeError here = header and library disagree
    want = "fp16" if flavour == "f16" else "bf16"
    if L.cn_operand16().decode() != want:
        raise HipError(f"{path}: the library's 16-bit operand is {L.cn_operand16().decode()}, expected {want}")
    _libs[path] = L
    return L


def check(rc, what="", L=None):
    """``L``: the library the failing call was made in (its cn_last_error() holds the message); default: the bf16 build."""
    if rc != 0:
        msg = (L or lib()).cn_last_error().decode(errors="replace")
        raise HipError(f"{what or 'libcassnat_hip'} failed (rc={rc}): {msg}")


def check_fp16_range(scores, what="decode"):
    """Second line behind ``Engine.check_range`` (which guards what the features' scale drives): a value beyond +-65504 in front of
    a matrix product INSIDE the layers - a matter of the checkpoint, not of the input - becomes an infinity; where that reaches a
    hypothesis score as a NaN the engine fails loudly instead of returning the hypothesis (a ReLU can still turn a NaN into a 0:
    a model whose activations leave the half range belongs on the bf16 engine)."""
    if not np.isfinite(np.asarray(scores, dtype=np.float64)).all():
        raise HipError(f"{what}: non-finite hypothesis score from the fp16 engine - an MFMA operand left the half-precision range "
                       "(+-65504); use --hip_precision bf16 / bf16x3 for this model or these features")


def subsampled(T):
    """T' of T frames after the two stride-2 convolutions (embedding.py:102-108)."""
    return ((T - 1) // 2 + 1 - 1) // 2 + 1


def _ptr(t):
    """Device/host pointer of a torch tensor (or None)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def current_stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cmvn_(feats, lens, mean, std):
    """In-place global CMVN of a padded (B, T, F) float32 CUDA batch on the current stream: frames t < lens[b] become
    float((double(x) - mean) / std) - SpeechDataset's arithmetic bit for bit (cn_op_cmvn); lens int32, mean / std float64, all
    on the batch's device."""
    B, T, F = feats.shape
    assert feats.is_contiguous() and feats.dtype.is_floating_point and feats.element_size() == 4 and lens.numel() >= B
    check(lib().cn_op_cmvn(_ptr(feats), _ptr(lens), _ptr(mean), _ptr(std), B, T, F, current_stream()), "cn_op_cmvn")
    return feats


def gather_offsets(sizes, align=1):
    """Byte offsets of pieces of ``sizes`` bytes laid one after the other, each starting on a multiple of ``align``, and the end
    of the last one."""
    sizes = np.asarray(sizes, dtype=np.uint64)
    a = np.uint64(max(1, int(align)))
    step = (sizes + (a - np.uint64(1))) // a * a
    offs = np.zeros(sizes.size, np.uint64)
    np.cumsum(step[:-1], out=offs[1:])
    return offs, int(offs[-1] + sizes[-1]) if sizes.size else 0


def host_gather(dst_ptr, srcs, threads=1, align=1):
    """Copy the numpy arrays ``srcs`` (C-contiguous; e.g. read-only views into a memory-mapped archive) to the host address
    ``dst_ptr`` in one GIL-free call (cn_host_gather), back to back - or, with ``align`` = a > 1, each piece at the next multiple
    of a bytes (the gaps are left as they are); returns the byte offsets of the pieces."""
    n = len(srcs)
    ptrs = np.fromiter((a.ctypes.data for a in srcs), np.uint64, n)
    sizes = np.fromiter((a.nbytes for a in srcs), np.uint64, n)
    offs, _ = gather_offsets(sizes, align)
    check(lib().cn_host_gather(C.c_void_p(int(dst_ptr)), ptrs.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p),
                               sizes.ctypes.data_as(C.c_void_p), n, int(threads)), "cn_host_gather")
    return offs


def unpack_rows(packed, off, lens, out, pad, mean=None, std=None):
    """The reader's collate on the device (cn_op_unpack_rows): ``packed`` float32 CUDA rows of F features, utterance r at row off[r]
    with lens[r] frames -> the padded (rows, T, F) batch ``out`` on the current stream; with ``mean`` / ``std`` (float64, (F,)) the
    global CMVN is applied in float64 on the way."""
    rows, T, F = out.shape
    assert out.is_contiguous() and packed.is_contiguous() and off.numel() >= rows and lens.numel() >= rows
    check(lib().cn_op_unpack_rows(_ptr(packed), _ptr(off), _ptr(lens), _ptr(out), rows, T, F, float(pad), _ptr(mean), _ptr(std),
                                  current_stream()), "cn_op_unpack_rows")
    return out


def unpack_compressed(staged, off, lens, kinds, out, pad, mean=None, std=None):
    """The reader's collate for Kaldi compressed matrices on the device (cn_op_unpack_compressed): ``staged`` uint8 CUDA bytes holding
    the archive payloads (``data.kaldi_io.mat_payload``: global header + data) of the utterances, payload r of kind kinds[r]
    (1 / 2 / 3 = CM / CM2 / CM3) with lens[r] rows at BYTE offset off[r], a multiple of 16 -> the padded (rows, T, F) batch ``out`` on
    the current stream, decompressed in Kaldi's float32 arithmetic; with ``mean`` / ``std`` (float64, (F,)) the global CMVN is
    applied in float64 on the way.  The caller has checked the payloads' headers against F, lens and their sizes."""
    rows, T, F = out.shape
    assert out.is_contiguous() and staged.is_contiguous() and staged.element_size() == 1
    assert off.numel() >= rows and lens.numel() >= rows and kinds.numel() >= rows
    check(lib().cn_op_unpack_compressed(_ptr(staged), _ptr(off), _ptr(lens), _ptr(kinds), _ptr(out), rows, T, F, float(pad), _ptr(mean),
                                        _ptr(std), current_stream()), "cn_op_unpack_compressed")
    return out


FEATS_STATUS = {1: "no rows", 2: "a non-finite value among its rows", 3: "its payload does not lie inside the output buffer"}


def compress_feats_bytes(T, F):
    """Bytes of the compressed payload of a T x F matrix (cn_compress_feats_bytes): `CM` for T > 8, `CM2` otherwise."""
    return int(lib().cn_compress_feats_bytes(int(T), int(F)))


def compress_feats_layout(lens, F, tmax=None):
    """Where ``compress_feats`` puts the payloads of utterances of ``lens`` rows (clamped to ``tmax``): (int32 byte offsets, multiples
    of 16; the payloads' sizes; the end of the last one)."""
    lens = np.asarray(lens, dtype=np.int64)
    T = np.maximum(lens if tmax is None else np.minimum(lens, int(tmax)), 0)
    sizes = np.where(T > 8, 16 + 8 * F + T * F, 16 + 2 * T * F)
    offs, total = gather_offsets(sizes, 16)
    if total >= 2 ** 31:
        raise ValueError("compress_feats_layout: %d payload bytes (the offsets are int32)" % total)
    return offs.astype(np.int32), sizes, total


def compress_feats(feats, lens, out_off, out, status, flavour=None):
    """Kaldi matrix compression on the device (cn_op_compress_feats; include/cassnat_hip_feats.h), the inverse of
    ``unpack_compressed``: ``feats`` float32 CUDA (rows, Tmax, F), ``lens`` int32 CUDA rows per utterance, ``out_off`` int32 CUDA byte
    offsets (``compress_feats_layout``) -> utterance r's payload at out[out_off[r]:] (``out`` uint8 CUDA, 16-byte aligned) and its
    status word in ``status`` (int32 CUDA; 0 fine, else ``FEATS_STATUS``), on the current stream.  Nothing else of ``out`` is written."""
    rows, T, F = feats.shape
    assert feats.is_contiguous() and feats.element_size() == 4 and out.is_contiguous() and out.element_size() == 1
    assert lens.numel() >= rows and out_off.numel() >= rows and status.numel() >= rows and status.element_size() == 4
    L = lib(flavour)
    check(L.cn_op_compress_feats(_ptr(feats), _ptr(lens), _ptr(out_off), rows, T, F, _ptr(out), out.numel(), _ptr(status), current_stream()),
          "cn_op_compress_feats", L)
    return out


def compress_feats_host(feats, lens, out_off, out, status, flavour=None):
    """``compress_feats`` on numpy arrays through the serial host entry (cn_compress_feats_host): no GPU call.  ``out`` (uint8) and
    ``status`` (int32) are written in place."""
    rows, T, F = feats.shape
    assert feats.dtype == np.float32 and feats.flags.c_contiguous and out.dtype == np.uint8 and out.flags.c_contiguous
    assert lens.dtype == np.int32 and out_off.dtype == np.int32 and status.dtype == np.int32 and min(lens.size, out_off.size, status.size) >= rows
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = lib(flavour)
    check(L.cn_compress_feats_host(p(feats), p(lens), p(out_off), rows, T, F, p(out), out.size, p(status)), "cn_compress_feats_host", L)
    return out


def feats_stats(feats, lens, stats, payload=None, out_off=None, status=None, flavour=None):
    """Per utterance and column the float64 sum and sum of squares of what an archive holds (cn_op_feats_stats) -> ``stats`` float64
    CUDA (rows, 2, F), on the current stream: with ``payload`` / ``out_off`` (what ``compress_feats`` wrote) the dequantised values,
    without them the float32 rows of ``feats`` (rows, Tmax, F).  An utterance whose ``status`` word is not 0 gives zeros.  No atomics:
    two runs give the same bits."""
    rows, T, F = feats.shape
    assert feats.is_contiguous() and feats.element_size() == 4 and stats.is_contiguous() and stats.element_size() == 8
    assert stats.numel() >= rows * 2 * F and lens.numel() >= rows and (payload is None or out_off is not None)
    L = lib(flavour)
    check(L.cn_op_feats_stats(_ptr(feats), _ptr(payload), _ptr(out_off), _ptr(lens), _ptr(status), rows, T, F, _ptr(stats), current_stream()),
          "cn_op_feats_stats", L)
    return stats


def feats_stats_host(feats, lens, payload=None, out_off=None, status=None, flavour=None):
    """``feats_stats`` on numpy arrays through the serial host entry (cn_feats_stats_host) -> float64 (rows, 2, F)."""
    rows, T, F = feats.shape
    assert feats.dtype == np.float32 and feats.flags.c_contiguous and lens.dtype == np.int32 and lens.size >= rows
    assert payload is None or (payload.dtype == np.uint8 and payload.flags.c_contiguous and out_off is not None and out_off.dtype == np.int32)
    assert status is None or status.dtype == np.int32
    stats = np.zeros((rows, 2, F), np.float64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    L = lib(flavour)
    check(L.cn_feats_stats_host(p(feats), p(payload), p(out_off), p(lens), p(status), rows, T, F, p(stats)), "cn_feats_stats_host", L)
    return stats


VAD_PARTS = abi.VAD_CONSTANTS["CN_VAD_PARTS"]


def frame_energy(staged, staged_bytes, off, samples, out_off, rows, N, shift, channels, channel, remove_dc, max_frames, num, e, flavour=None):
    """Per-frame integer energies of staged int16 audio on the device (cn_op_frame_energy; include/cassnat_hip_vad.h): ``staged`` uint8
    CUDA bytes, row r a run of samples[r] sample frames of ``channels`` interleaved channels at BYTE offset off[r] (a multiple of 16);
    frame t of row r -> index out_off[r] + t of ``num`` (int64 CUDA) and ``e`` (float64 CUDA: the log-energy), at most ``max_frames``
    frames per row, on the current stream.  ``off`` / ``samples`` / ``out_off`` int32 CUDA.  Nothing else is written."""
    assert staged.is_contiguous() and staged.element_size() == 1 and 0 <= int(staged_bytes) <= staged.numel()
    assert min(off.numel(), samples.numel(), out_off.numel()) >= rows and num.element_size() == 8 and e.element_size() == 8
    L = lib(flavour)
    check(L.cn_op_frame_energy(_ptr(staged), int(staged_bytes), _ptr(off), _ptr(samples), _ptr(out_off), int(rows), int(N), int(shift),
                               int(channels), int(channel), int(bool(remove_dc)), int(max_frames), _ptr(num), _ptr(e), current_stream()),
          "cn_op_frame_energy", L)
    return num, e


def frame_energy_host(staged, off, samples, out_off, N, shift, channels, channel, remove_dc, max_frames, num, e, staged_bytes=None, flavour=None):
    """``frame_energy`` on numpy arrays through the serial host entry (cn_frame_energy_host): no GPU call.  ``num`` (int64) and ``e``
    (float64) are written in place."""
    assert staged.dtype == np.uint8 and staged.flags.c_contiguous and num.dtype == np.int64 and e.dtype == np.float64
    assert off.dtype == np.int32 and samples.dtype == np.int32 and out_off.dtype == np.int32 and off.size == samples.size == out_off.size
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = lib(flavour)
    check(L.cn_frame_energy_host(p(staged), staged.size if staged_bytes is None else int(staged_bytes), p(off), p(samples), p(out_off), off.size,
                                 int(N), int(shift), int(channels), int(channel), int(bool(remove_dc)), int(max_frames), p(num), p(e)),
          "cn_frame_energy_host", L)
    return num, e


def vad_decide(e, rec_off, rec_frames, recs, thr0, mean_scale, context, proportion, thr, dec, flavour=None):
    """Kaldi's energy VAD decision on the device (cn_op_vad_decide): recording i holds the frames e[rec_off[i] : rec_off[i] +
    rec_frames[i]] (``e`` float64 CUDA, the offsets and counts int32 CUDA) -> ``dec`` (uint8 CUDA, one byte per frame at the frames'
    indices) and ``thr`` (float64 CUDA of at least recs * (1 + VAD_PARTS): the thresholds first, the partial sums behind them), on the
    current stream."""
    assert e.element_size() == 8 and thr.element_size() == 8 and thr.numel() >= recs * (1 + VAD_PARTS) and dec.element_size() == 1
    assert min(rec_off.numel(), rec_frames.numel()) >= recs
    L = lib(flavour)
    check(L.cn_op_vad_decide(_ptr(e), _ptr(rec_off), _ptr(rec_frames), int(recs), float(thr0), float(mean_scale), int(context),
                             float(proportion), _ptr(thr), _ptr(dec), current_stream()), "cn_op_vad_decide", L)
    return thr, dec


def vad_decide_host(e, rec_off, rec_frames, thr0, mean_scale, context, proportion, thr, dec, flavour=None):
    """``vad_decide`` on numpy arrays through the serial host entry (cn_vad_decide_host): ``thr`` (float64, one per recording) and
    ``dec`` (uint8) are written in place."""
    assert e.dtype == np.float64 and thr.dtype == np.float64 and dec.dtype == np.uint8 and rec_off.dtype == np.int32 and rec_frames.dtype == np.int32
    assert rec_off.size == rec_frames.size <= thr.size
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = lib(flavour)
    check(L.cn_vad_decide_host(p(e), p(rec_off), p(rec_frames), rec_off.size, float(thr0), float(mean_scale), int(context), float(proportion),
                               p(thr), p(dec)), "cn_vad_decide_host", L)
    return thr, dec


def splice_rows(src, off, lens, out, left, right, skip, pad, mean=None, std=None):
    """Frame splicing and skipping on the device (cn_op_splice_rows): ``src`` float32 CUDA rows of F0 features, utterance r at row
    off[r] with lens[r] rows -> ``out`` (rows, T_out, (left + right + 1) * F0) on the current stream: the dataset's order - CMVN
    (``mean`` / ``std`` float64 (F0,), when given), zero rows up to a multiple of ``skip``, ``feat_op.context_feat`` with replicated
    edges, ``feat_op.skip_feat`` - then collate's padding.  ``src`` may be the packed archive rows of a pass, or a padded, already
    normalised (rows, T0, F0) batch with off[r] = r * T0 (rows at or behind lens[r] are never read)."""
    rows, T, W = out.shape
    blocks = int(left) + int(right) + 1
    assert blocks >= 1 and W % blocks == 0, "splice_rows: the output width is not (left + right + 1) x F0"
    assert out.is_contiguous() and src.is_contiguous() and out.element_size() == 4 and src.element_size() == 4
    assert off.numel() >= rows and lens.numel() >= rows
    check(lib().cn_op_splice_rows(_ptr(src), _ptr(off), _ptr(lens), _ptr(out), rows, T, W // blocks, int(left), int(right), int(skip),
                                  float(pad), _ptr(mean), _ptr(std), current_stream()), "cn_op_splice_rows")
    return out


def fbank_packed(opts, staged, staged_bytes, off, samples, out, pad, mean=None, std=None):
    """The Kaldi fbank front-end behind the packed reader (cn_op_fbank_packed): ``staged`` uint8 CUDA bytes holding the utterances'
    little-endian int16 samples as the WAV `data` chunks hold them, utterance r with samples[r] samples at BYTE offset off[r], a
    multiple of 16 -> the padded (rows, T, num_mel) batch ``out`` on the current stream: frame t < num_frames(samples[r]) is
    ``cn_fbank``'s value bit for bit, later frames are ``pad``; with ``mean`` / ``std`` (float64, (num_mel,)) the global CMVN is
    applied in float64 on the way.  ``opts``: a ``CnFbankOpts``."""
    rows, T, F = out.shape
    assert out.is_contiguous() and out.element_size() == 4 and staged.is_contiguous() and staged.element_size() == 1
    assert F == opts.num_mel and 0 <= int(staged_bytes) <= staged.numel() and off.numel() >= rows and samples.numel() >= rows
    check(lib().cn_op_fbank_packed(opts, _ptr(staged), int(staged_bytes), _ptr(off), _ptr(samples), _ptr(out), rows, T, float(pad),
                                   _ptr(mean), _ptr(std), current_stream()), "cn_op_fbank_packed")
    return out


def fbank_packed_f32(opts, wave, wave_bytes, off, samples, out, pad, mean=None, std=None):
    """``fbank_packed`` for float32 samples on the int16 scale (cn_op_fbank_packed_f32): ``wave`` float32 CUDA, utterance r with
    samples[r] samples at BYTE offset off[r], a multiple of 16 - the wave ``wave_resample`` wrote.  Same kernel, same values bit for
    bit for the same samples."""
    rows, T, F = out.shape
    assert out.is_contiguous() and out.element_size() == 4 and wave.is_contiguous() and wave.element_size() == 4
    assert F == opts.num_mel and 0 <= int(wave_bytes) <= 4 * wave.numel() and off.numel() >= rows and samples.numel() >= rows
    check(lib().cn_op_fbank_packed_f32(opts, _ptr(wave), int(wave_bytes), _ptr(off), _ptr(samples), _ptr(out), rows, T, float(pad),
                                       _ptr(mean), _ptr(std), current_stream()), "cn_op_fbank_packed_f32")
    return out


def resample_num_samples(in_rate, out_rate, samples):
    """Outputs of Kaldi's LinearResample for ``samples`` inputs, flushed (cn_resample_num_samples; host only)."""
    return int(lib().cn_resample_num_samples(int(in_rate), int(out_rate), int(samples)))


def resample_table(in_rate, out_rate):
    """The weight table of a rate pair exactly as the device gets it (cn_resample_table; host only) -> dict: ``in_unit``, ``out_unit``
    (the phases), ``max_taps``, ``first`` / ``taps`` int32 (out_unit,), ``weights`` float32 (max_taps, out_unit), zero behind a
    phase's taps."""
    iu, ou, mt = C.c_int32(), C.c_int32(), C.c_int32()
    L = lib()
    check(L.cn_resample_table(int(in_rate), int(out_rate), C.byref(iu), C.byref(ou), C.byref(mt), None, None, None, 0), "cn_resample_table")
    first, taps = np.zeros(ou.value, np.int32), np.zeros(ou.value, np.int32)
    weights = np.zeros((mt.value, ou.value), np.float32)
    check(L.cn_resample_table(int(in_rate), int(out_rate), C.byref(iu), C.byref(ou), C.byref(mt), first.ctypes.data_as(C.c_void_p),
                              taps.ctypes.data_as(C.c_void_p), weights.ctypes.data_as(C.c_void_p), weights.size), "cn_resample_table")
    return {"in_unit": iu.value, "out_unit": ou.value, "max_taps": mt.value, "first": first, "taps": taps, "weights": weights}


def wave_resample(in_rate, out_rate, staged, staged_bytes, off, samples, channels, channel, channels_host, channel_host, wave, out_off,
                  max_out, rows=None, n_rows=None):
    """Sample-rate conversion and channel pick on the device (cn_op_wave_resample), the utterances of ONE source rate: ``staged``
    uint8 CUDA bytes holding the data chunks as the files hold them (interleaved int16; utterance r: channels[r] channels of
    samples[r] samples at BYTE offset off[r], a multiple of 16) -> channel channel[r] at ``out_rate``, float32, written to ``wave``
    from float offset out_off[r] on: ``resample_num_samples`` values, nothing else.  ``rows`` (int32 CUDA): the utterances of this
    call (None: the first ``n_rows``, default all); ``max_out``: their longest output count.  ``channels_host`` / ``channel_host``:
    int32 numpy arrays of the same values, checked before the launch."""
    utts = int(channels_host.shape[0])
    assert staged.is_contiguous() and staged.element_size() == 1 and 0 <= int(staged_bytes) <= staged.numel()
    assert wave.is_contiguous() and wave.element_size() == 4
    assert channels_host.dtype == np.int32 and channel_host.dtype == np.int32 and channel_host.shape[0] == utts
    assert channels_host.flags.c_contiguous and channel_host.flags.c_contiguous
    assert min(off.numel(), samples.numel(), channels.numel(), channel.numel(), out_off.numel()) >= utts
    n = int(rows.numel() if rows is not None and n_rows is None else (utts if n_rows is None else n_rows))
    assert rows is None or rows.numel() >= n
    check(lib().cn_op_wave_resample(int(in_rate), int(out_rate), _ptr(staged), int(staged_bytes), _ptr(off), _ptr(samples), _ptr(channels),
                                    _ptr(channel), channels_host.ctypes.data_as(C.c_void_p), channel_host.ctypes.data_as(C.c_void_p), utts,
                                    _ptr(rows), n, int(max_out), _ptr(wave), _ptr(out_off), current_stream()), "cn_op_wave_resample")
    return wave


class FlacIndexError(ValueError):
    """``flac_index`` refused a stream: ``code`` is cn_host_flac_index's (-2 no chain of frames, -3 a frame unlike STREAMINFO, -6 out of
    range), ``offset`` the byte offset it names."""

    def __init__(self, msg, code, offset):
        super().__init__(msg)
        self.code, self.offset = code, offset


def flac_index(audio, rate, channels, bits=16, frames_hint=0):
    """The exact frame index of a FLAC stream's audio bytes (cn_host_flac_index; host only, GIL-free): ``audio`` a C-contiguous uint8
    array from the first frame to the end of the file -> (int32 (frames, 3): byte offset, byte length, first sample; total samples).
    A stream in which no chain of frames with matching CRC-16s reaches the end, or a frame of which differs from (rate, channels,
    bits), raises ``FlacIndexError``."""
    assert audio.dtype == np.uint8 and audio.ndim == 1 and audio.flags.c_contiguous
    L = lib()
    nf, ns, bad = C.c_int64(), C.c_int64(), C.c_int64()
    cap = int(frames_hint) + 16 if frames_hint else audio.shape[0] // 256 + 16
    while True:
        out = np.empty((cap, 3), np.int32)
        rc = L.cn_host_flac_index(C.c_void_p(audio.ctypes.data), audio.shape[0], int(rate), int(channels), int(bits), C.c_void_p(out.ctypes.data), cap,
                                  C.byref(nf), C.byref(ns), C.byref(bad))
        if rc != -5:
            break
        cap = max(2 * cap, audio.shape[0] // 9 + 1) if cap < audio.shape[0] // 9 + 1 else cap * 2  # (a frame takes at least 9 bytes)
    if rc != 0:
        raise FlacIndexError(L.cn_last_error().decode(errors="replace").replace("cn_host_flac_index: ", ""), rc, bad.value)
    return out[:nf.value].copy(), int(ns.value)


def flac_crc16(data):
    """CRC-16 of a FLAC frame's bytes (cn_host_flac_crc16; host only)."""
    data = bytes(data)
    return int(lib().cn_host_flac_crc16(data, len(data)))


def flac_frame_words(channels, block_size):
    """Scratch words of one frame in ``flac_decode`` (cn_flac_frame_words)."""
    return int(lib().cn_flac_frame_words(int(channels), int(block_size)))


def flac_scratch_bytes(frames, frame_words):
    return int(lib().cn_flac_scratch_bytes(int(frames), int(frame_words)))


def flac_decode(staged, staged_bytes, table, frames, utt, utts, max_channels, frame_words, pcm, pcm_bytes, status, scratch=None):
    """FLAC frames -> interleaved int16 PCM on the device (cn_op_flac_decode), on the current stream: ``staged`` uint8 CUDA bytes of
    the files, ``table`` int32 CUDA (frames, 4) - byte offset, byte length, utterance, first sample -, ``utt`` int32 CUDA (3, utts) -
    channels, samples per channel, byte offset of the PCM in ``pcm`` (uint8 CUDA) -, ``status`` one int32 CUDA word: 0 after a clean
    pass, else a failed frame's index + 1.  ``scratch``: a CUDA buffer of ``flac_scratch_bytes`` bytes - None: the call allocates
    one and waits for the stream."""
    assert staged.is_contiguous() and staged.element_size() == 1 and 0 <= int(staged_bytes) <= staged.numel()
    assert table.is_contiguous() and table.element_size() == 4 and table.numel() >= 4 * int(frames)
    assert utt.is_contiguous() and utt.element_size() == 4 and utt.numel() >= 3 * int(utts)
    assert pcm.is_contiguous() and 0 <= int(pcm_bytes) <= pcm.numel() * pcm.element_size() and status.element_size() == 4
    check(lib().cn_op_flac_decode(_ptr(staged), int(staged_bytes), _ptr(table), int(frames), _ptr(utt), int(utts), int(max_channels),
                                  int(frame_words), _ptr(pcm), int(pcm_bytes), _ptr(status), _ptr(scratch),
                                  0 if scratch is None else scratch.numel() * scratch.element_size(), current_stream()), "cn_op_flac_decode")
    return pcm


EDIT_OPS = "CSDI"  # the codes of an edit path: 0 correct, 1 substituted, 2 deleted, 3 inserted


def edit_align(ref, ref_begin, ref_len, hyp, hyp_begin, hyp_len, costs=(1, 1, 1), max_ref=None, max_hyp=None, bp_lds_limit=-1, flavour=None):
    """Weighted edit alignment of N pairs of id sequences on the device (cn_op_edit_align; include/cassnat_hip_score.h): ``ref`` /
    ``hyp`` int32 CUDA id arrays, pair n = ref[ref_begin[n] .. + ref_len[n]) against hyp[hyp_begin[n] .. + hyp_len[n]) (begins int64,
    lengths int32, CUDA; pairs may share a reference), ``costs`` = (sub, ins, del).  ``max_ref`` / ``max_hyp`` clamp the lengths and
    size the launch (None: the largest length, which costs a copy to the host).  -> (cost (N,) int32, counts (N, 4) int32 C / S / D / I,
    path_len (N,) int32, ops uint8, ops_begin (N,) int64) as CUDA tensors: pair n's path is ops[ops_begin[n] .. + path_len[n]), codes
    as in ``EDIT_OPS``.  On the current stream; returns once it has drained."""
    import torch

    dev = ref.device
    ref, hyp = ref.to(dev, torch.int32).contiguous(), hyp.to(dev, torch.int32).contiguous()
    ref_begin, hyp_begin = ref_begin.to(dev, torch.int64).contiguous(), hyp_begin.to(dev, torch.int64).contiguous()
    ref_len, hyp_len = ref_len.to(dev, torch.int32).contiguous(), hyp_len.to(dev, torch.int32).contiguous()
    N = int(ref_len.numel())
    assert ref_begin.numel() == N and hyp_begin.numel() == N and hyp_len.numel() == N
    if N and (max_ref is None or max_hyp is None):
        mr, mh = torch.stack([ref_len.max(), hyp_len.max()]).tolist()
        max_ref, max_hyp = (max(0, mr) if max_ref is None else max_ref), (max(0, mh) if max_hyp is None else max_hyp)
    max_ref, max_hyp = int(max_ref or 0), int(max_hyp or 0)
    span = ref_len.clamp(0, max(0, max_ref)).to(torch.int64) + hyp_len.clamp(0, max(0, max_hyp)).to(torch.int64)
    ops_begin = torch.cumsum(span, 0) - span
    ops_total = int(span.sum().item()) if N else 0
    ops = torch.zeros(max(1, ops_total), dtype=torch.uint8, device=dev)
    cost = torch.zeros(max(1, N), dtype=torch.int32, device=dev)
    counts = torch.zeros(max(1, N), 4, dtype=torch.int32, device=dev)
    plen = torch.zeros(max(1, N), dtype=torch.int32, device=dev)
    L = lib(flavour)
    # (an empty id array still needs an address: the op refuses null buffers)
    refp, hypp = (t if t.numel() else torch.zeros(1, dtype=torch.int32, device=dev) for t in (ref, hyp))
    check(L.cn_op_edit_align(_ptr(refp), ref.numel(), _ptr(ref_begin), _ptr(ref_len), _ptr(hypp), hyp.numel(), _ptr(hyp_begin), _ptr(hyp_len), N,
                             max_ref, max_hyp, int(costs[0]), int(costs[1]), int(costs[2]), int(bp_lds_limit), _ptr(cost), _ptr(counts), _ptr(plen),
                             _ptr(ops), ops_total, _ptr(ops_begin), current_stream()), "cn_op_edit_align", L)
    return cost[:N], counts[:N], plen[:N], ops[:ops_total], ops_begin


def edit_align_host(ref, ref_begin, ref_len, hyp, hyp_begin, hyp_len, costs=(1, 1, 1), max_ref=None, max_hyp=None, flavour=None):
    """``edit_align`` on numpy arrays through the serial host entry (cn_edit_align_host): no GPU call.  Same outputs, as numpy arrays."""
    ref, hyp = np.ascontiguousarray(ref, np.int32).reshape(-1), np.ascontiguousarray(hyp, np.int32).reshape(-1)
    ref_begin, hyp_begin = np.ascontiguousarray(ref_begin, np.int64).reshape(-1), np.ascontiguousarray(hyp_begin, np.int64).reshape(-1)
    ref_len, hyp_len = np.ascontiguousarray(ref_len, np.int32).reshape(-1), np.ascontiguousarray(hyp_len, np.int32).reshape(-1)
    N = int(ref_len.size)
    assert ref_begin.size == N and hyp_begin.size == N and hyp_len.size == N
    max_ref = int(max(0, ref_len.max(initial=0)) if max_ref is None else max_ref)
    max_hyp = int(max(0, hyp_len.max(initial=0)) if max_hyp is None else max_hyp)
    span = np.clip(ref_len, 0, max(0, max_ref)).astype(np.int64) + np.clip(hyp_len, 0, max(0, max_hyp)).astype(np.int64)
    ops_begin = np.cumsum(span) - span
    ops_total = int(span.sum())
    ops = np.zeros(max(1, ops_total), np.uint8)
    cost, counts, plen = np.zeros(max(1, N), np.int32), np.zeros((max(1, N), 4), np.int32), np.zeros(max(1, N), np.int32)
    refp, hypp = (a if a.size else np.zeros(1, np.int32) for a in (ref, hyp))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    L = lib(flavour)
    check(L.cn_edit_align_host(p(refp), ref.size, p(ref_begin), p(ref_len), p(hypp), hyp.size, p(hyp_begin), p(hyp_len), N, max_ref, max_hyp,
                               int(costs[0]), int(costs[1]), int(costs[2]), p(cost), p(counts), p(plen), p(ops), ops_total, p(ops_begin)),
          "cn_edit_align_host", L)
    return cost[:N], counts[:N], plen[:N], ops[:ops_total], ops_begin


# ---- AST beam search with phrase biasing: the three kernels alone (include/cassnat_hip_ast_bias.h), on the current stream
def ast_bias_nodes(desc, tok, lens, flavour=None):
    """The automaton node of every row of ``tok`` int32 (n, ld) cuda, rows WITHOUT sos, ``lens`` int32 (n,) -> int32 (n,) cuda."""
    import torch

    out = torch.empty(tok.shape[0], dtype=torch.int32, device=tok.device)
    L = lib(flavour)
    check(L.cn_op_ast_bias_nodes(C.byref(desc), _ptr(tok), tok.shape[1], _ptr(lens), tok.shape[0], _ptr(out), current_stream()),
          "cn_op_ast_bias_nodes", L)
    return out


def ast_bias_terms(desc, node, eos, idx, flavour=None):
    """The terms of the candidates ``idx`` int32 (n, K) cuda for hypotheses at ``node`` int32 (n,) -> float32 (n, K) cuda."""
    import torch

    out = torch.empty(idx.shape, dtype=torch.float32, device=idx.device)
    L = lib(flavour)
    check(L.cn_op_ast_bias_terms(C.byref(desc), _ptr(node), int(eos), _ptr(idx), idx.shape[0], idx.shape[1], _ptr(out), current_stream()),
          "cn_op_ast_bias_terms", L)
    return out


def logsoftmax_bias_topk(att, temperature, desc, node, eos, k, flavour=None):
    """Per row of ``att`` float32 (M, V) cuda the k best of log_softmax(att / T) + term -> (idx int32 (M, k), val float32 (M, k))."""
    import torch

    M, V = att.shape
    idx = torch.empty(M, k, dtype=torch.int32, device=att.device)
    val = torch.empty(M, k, dtype=torch.float32, device=att.device)
    L = lib(flavour)
    check(L.cn_op_logsoftmax_bias_topk(_ptr(att), M, V, float(temperature), C.byref(desc), _ptr(node), int(eos), int(k), _ptr(idx), _ptr(val),
                                       current_stream()), "cn_op_logsoftmax_bias_topk", L)
    return idx, val


class Engine:
    """Owns one ``cn_model`` handle: weights, workspace and the decode pipeline on one GPU."""

    def __init__(self, args, precision="bf16", max_batch=32, max_frames=2048, device=0, esa_group=1, share_with=None):
        """``share_with``: a finalized Engine of the same model - the new handle uses ITS device copy of the packed weights
        (reference counted in the library) and only allocates a workspace of its own; it is ready to decode."""
        self.L = lib_for(precision)
        ast = int(getattr(args, "ast", 0))
        self.cfg = CnConfig(
            input_size=args.input_size, d_model=args.d_model, n_head=args.n_head, d_encff=args.d_encff,
            d_decff=args.d_decff, n_enc=args.N_enc, n_extra=args.N_extra, n_self_dec=args.N_self_dec,
            n_mix_dec=args.N_mix_dec, vocab_size=args.vocab_size, precision=PRECISION[precision],
            max_batch=max_batch, max_frames=max_frames, device=device, ast=ast,
            conf_enc=int(getattr(args, "conf_enc", 0)), conf_dec=int(getattr(args, "conf_dec", 0)),
            enc_max_rel=int(getattr(args, "enc_max_rel", 0)), dec_max_rel=int(getattr(args, "dec_max_rel", 0)),
            enc_kernel=int(getattr(args, "enc_kernel", 0)), dec_kernel=int(getattr(args, "dec_kernel", 0)),
            d_ff=int(getattr(args, "d_ff", 0)), esa_group=int(esa_group),
            fp8_scope=int(getattr(args, "fp8_scope", 0)), fp8_ffn_first_layer=int(getattr(args, "fp8_ffn_first_layer", 0)))
        self.precision = precision
        self.handle = C.c_void_p()
        if share_with is not None:
            if not share_with.finalized or not share_with.handle:
                raise HipError("share_with needs a finalized engine")
            self._chk(self.L.cn_model_create_shared(C.byref(self.cfg), share_with.handle, C.byref(self.handle)), "cn_model_create_shared")
            self.finalized = True
        else:
            self._chk(self.L.cn_model_create(C.byref(self.cfg), C.byref(self.handle)), "cn_model_create")
            self.finalized = False

    def _chk(self, rc, what=""):
        check(rc, what, self.L)

    def close(self):
        if getattr(self, "handle", None):
            self.L.cn_model_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state(self, state, pe_table):
        """state: name -> float32 array/tensor (reference parameter names); pe_table: (rows, d_model)."""
        for name, w in state.items():
            a = np.ascontiguousarray(w.detach().cpu().numpy() if hasattr(w, "detach") else w, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._chk(self.L.cn_model_load_weights(self.handle, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim),
                  f"load {name}")
        pe = np.ascontiguousarray(pe_table.detach().cpu().numpy() if hasattr(pe_table, "detach") else pe_table,
                                  dtype=np.float32)
        self._chk(self.L.cn_model_load_pe(self.handle, pe.ctypes.data_as(C.c_void_p), pe.shape[0]), "load pe")
        self.finalize()

    def finalize(self):
        self._chk(self.L.cn_model_finalize(self.handle), "cn_model_finalize")
        self.finalized = True

    def weight_blob(self):
        """(device pointer, bytes) of the packed weights - what RCCL broadcasts from rank 0."""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.cn_model_weight_blob(self.handle, C.byref(p), C.byref(n)), "cn_model_weight_blob")
        return p.value, n.value

    @staticmethod
    def make_opts(args, capture=False):
        # (an autoregressive model's args carry no trigger options: ctc_beam_decode runs on either kind of model)
        # args.hip_padded_rows: cn_decode_opts.reserved[1] - the decoder side on padded [B][U] rows where it would pack each
        # utterance's own rows (same results bit for bit; the A/B switch of the two layouts)
        opts = CnDecodeOpts(padding_idx=int(args.padding_idx), sos=1, left_trigger=int(getattr(args, "left_trigger", 0)),
                            right_trigger=int(getattr(args, "right_trigger", 0)), src_trigger=int(bool(getattr(args, "src_trigger", False))),
                            use_unimask=int(bool(getattr(args, "use_unimask", False))), beam_width=int(args.beam_width),
                            capture=int(bool(capture)), no_trigger=int(not getattr(args, "use_trigger", True)))
        opts.reserved[1] = int(bool(getattr(args, "hip_padded_rows", False)))
        # args.hip_chain_qkv: cn_decode_opts.reserved[2] - the encoder's Q|K|V written by the row-chain launches where the
        # self-attention kernel would project them itself (same results bit for bit; the A/B switch of the two forms)
        opts.reserved[2] = int(bool(getattr(args, "hip_chain_qkv", False)))
        return opts

    def decode(self, feats, size_ratio, opts, hyp, hyp_len, score):
        """feats (B,T,F) f32 cuda, size_ratio (B,) f32 cuda; outputs are caller-owned cuda tensors."""
        B, T, F = feats.shape
        self._chk(self.L.cn_decode_nast(self.handle, _ptr(feats), _ptr(size_ratio), B, T, F, C.byref(opts), _ptr(hyp),
                                    hyp.shape[1], _ptr(hyp_len), _ptr(score), current_stream()), "cn_decode_nast")

    def decode_merged(self, feats, size_ratio, opts, sub_rows, sub_frames, hyp, hyp_len, score, u_hint=0):
        """One engine pass over several reference batches (``cn_decode_nast_merged``): ``feats`` (B, T, F) holds the batches one
        after the other, batch k = ``sub_rows[k]`` utterances of ``sub_frames[k]`` <= T frames (padded to T with padding_idx
        frames); every utterance's result is that of a pass of its own batch.  ``sub_rows`` empty / None: a plain call.
        ``u_hint`` > 0: no mid-pass host sync - the decoder side runs on that many rows; returns the ticket whose
        ``ticket(t) -> (ymax, rows_used)`` the caller reads once the stream has drained (rows_used < ymax: decode again)."""
        B, T, F = feats.shape
        n = len(sub_rows) if sub_rows is not None else 0
        rows = (C.c_int32 * max(1, n))(*[int(x) for x in (sub_rows or [])])
        frames = (C.c_int32 * max(1, n))(*[int(x) for x in (sub_frames or [])])
        ticket = C.c_int32(-1)
        self._chk(self.L.cn_decode_nast_merged(self.handle, _ptr(feats), _ptr(size_ratio), B, T, F, C.byref(opts), n, rows, frames,
                                           int(u_hint), _ptr(hyp), hyp.shape[1], _ptr(hyp_len), _ptr(score), current_stream(),
                                           C.byref(ticket)), "cn_decode_nast_merged")
        return ticket.value

    def check_range(self, what="decode"):
        """fp16 engines: raise if a pass since the last call saw features beyond the range the half-precision operands hold
        (``cn_take_range_fault``; call it once the passes' results are on the host).  Other engines: nothing to check."""
        if self.precision not in ("fp16", "float16", "bf16x3"):
            return
        fault, limit = C.c_int32(), C.c_float()
        self._chk(self.L.cn_take_range_fault(self.handle, C.byref(fault), C.byref(limit)), "cn_take_range_fault")
        if fault.value and self.precision == "bf16x3":
            raise HipError(f"{what}: features beyond the range the split-bf16 engine's mixed-arithmetic convolution holds at its "
                           f"tolerance (|x| > {limit.value:.4g} lets conv1 outputs pass the e4m3 operands' 448): normalise the features "
                           "(CMVN) or decode with --hip_precision fp32")
        if fault.value:
            raise HipError(f"{what}: features beyond the fp16 engine's half-precision range (|x| > {limit.value:.4g} lets a subsampling "
                           "convolution's output pass 65504 / 2): normalise the features (CMVN) or decode with --hip_precision bf16 / bf16x3")

    def ticket(self, t):
        """(true row count, rows the decoder side ran on) of the pass that returned ticket ``t``; valid once its stream work is done."""
        ymax, used = C.c_int32(), C.c_int32()
        self._chk(self.L.cn_decode_ticket(self.handle, int(t), C.byref(ymax), C.byref(used)), "cn_decode_ticket")
        return ymax.value, used.value

    def encode_align(self, feats, size_ratio, opts):
        B, T, F = feats.shape
        ymax = C.c_int32()
        self._chk(self.L.cn_encode_align(self.handle, _ptr(feats), _ptr(size_ratio), B, T, F, C.byref(opts),
                                     C.byref(ymax), current_stream()), "cn_encode_align")
        return ymax.value

    # ---- autoregressive (AST) path
    def ast_begin(self, feats, opts, want_ctc, max_len, max_slots, ctc_beam):
        B, T, F = feats.shape
        self._chk(self.L.cn_ast_begin(self.handle, _ptr(feats), B, T, F, C.byref(opts), int(want_ctc), max_len, max_slots,
                                  ctc_beam, current_stream()), "cn_ast_begin")

    def ast_step(self, pos, tok, utt, anc, keyok, temperature, K, topk_idx, topk_val):
        self._chk(self.L.cn_ast_step(self.handle, tok.shape[0], pos, _ptr(tok), _ptr(utt), _ptr(anc), _ptr(keyok), anc.shape[1],
                                 float(temperature), K, _ptr(topk_idx), _ptr(topk_val), current_stream()), "cn_ast_step")

    def ast_attach_lm(self, lm):
        """LM shallow fusion: ``lm`` (an Engine of a TransformerLM, same library) runs beside this engine's decoder steps; None
        detaches.  The caller keeps ``lm`` open while attached."""
        if lm is not None and lm.L is not self.L:
            raise HipError("cn_ast_attach_lm: the LM engine comes from the other library")
        self._chk(self.L.cn_ast_attach_lm(self.handle, lm.handle if lm is not None else None), "cn_ast_attach_lm")
        self._lm = lm

    def ast_step_lm(self, pos, tok, utt, anc, keyok, temperature, K, lm_weight, use_ctc, topk_idx, topk_val, lm_val=None):
        self._chk(self.L.cn_ast_step_lm(self.handle, tok.shape[0], pos, _ptr(tok), _ptr(utt), _ptr(anc), _ptr(keyok), anc.shape[1],
                                    float(temperature), K, float(lm_weight), int(use_ctc), _ptr(topk_idx), _ptr(topk_val),
                                    _ptr(lm_val) if lm_val is not None else None, current_stream()), "cn_ast_step_lm")

    def ast_attach_ngram(self, desc, lm_scale=0.0):
        """Word n-gram shallow fusion (include/cassnat_hip_ast_ngram.h): ``desc`` a ``CnNgramDesc`` over tables on this engine's
        device (copied; the caller keeps the tables alive while attached), ``lm_scale`` = float32(lm_weight * ln 10); None detaches."""
        self._chk(self.L.cn_ast_attach_ngram(self.handle, C.byref(desc) if desc is not None else None, float(lm_scale)),
                  "cn_ast_attach_ngram")

    def ast_step_ngram(self, pos, tok, utt, anc, keyok, temperature, K, use_ctc, eos, adds, topk_idx, topk_val, term=None):
        """``ast_step`` with the attached n-gram model: ``adds`` float32 (n, 2) cuda.  Without CTC topk_idx / topk_val are the fused
        top-K; with CTC they are the attention top-K and ``term`` (n, K) receives the terms at it."""
        self._chk(self.L.cn_ast_step_ngram(self.handle, tok.shape[0], pos, _ptr(tok), _ptr(utt), _ptr(anc), _ptr(keyok), anc.shape[1],
                                           float(temperature), K, int(use_ctc), int(eos), _ptr(adds), _ptr(topk_idx), _ptr(topk_val),
                                           _ptr(term) if term is not None else None, current_stream()), "cn_ast_step_ngram")

    def ast_attach_bias(self, desc):
        """Contextual phrase biasing (include/cassnat_hip_ast_bias.h): ``desc`` a ``CnBiasDesc`` over tables on this engine's device
        (copied; the caller keeps the tables alive while attached); None detaches."""
        self._chk(self.L.cn_ast_attach_bias(self.handle, C.byref(desc) if desc is not None else None), "cn_ast_attach_bias")

    def ast_step_bias(self, pos, tok, utt, anc, keyok, temperature, K, use_ctc, eos, node, topk_idx, topk_val, term=None):
        """``ast_step`` with the attached phrase list: ``node`` int32 (n,) cuda.  Without CTC topk_idx / topk_val are the fused
        top-K; with CTC they are the attention top-K and ``term`` (n, K) receives the terms at it."""
        self._chk(self.L.cn_ast_step_bias(self.handle, tok.shape[0], pos, _ptr(tok), _ptr(utt), _ptr(anc), _ptr(keyok), anc.shape[1],
                                          float(temperature), K, int(use_ctc), int(eos), _ptr(node), _ptr(topk_idx), _ptr(topk_val),
                                          _ptr(term) if term is not None else None, current_stream()), "cn_ast_step_bias")

    # ---- CASS-NAT + LM: the finish loop with LM shallow fusion
    def nat_attach_lm(self, lm):
        """``lm`` (an Engine of a TransformerLM, same library) is the lm_model of this NAT engine's fused finish loop; None
        detaches.  The caller keeps ``lm`` open while attached."""
        if lm is not None and lm.L is not self.L:
            raise HipError("cn_nat_attach_lm: the LM engine comes from the other library")
        self._chk(self.L.cn_nat_attach_lm(self.handle, lm.handle if lm is not None else None), "cn_nat_attach_lm")
        self._lm = lm

    def nat_lm_finish(self, opts, ymax, beam_width, lm_weight, length_penalty, zero_past_len, hyp, hyp_len, score):
        """The finish loop with the attached LM after a pass that kept its rows (``opts.reserved[0] = 1``): hyp int32
        (B, beam, max_len), hyp_len int32 (B, beam), score float64 (B, beam) cuda tensors; ``length_penalty`` None sorts on the score."""
        self._chk(self.L.cn_nat_lm_finish(self.handle, C.byref(opts), int(ymax), int(beam_width), float(lm_weight),
                                          int(length_penalty is not None), float(length_penalty or 0.0), int(bool(zero_past_len)),
                                          _ptr(hyp), hyp.shape[2], _ptr(hyp_len), _ptr(score), current_stream()), "cn_nat_lm_finish")

    # ---- CASS-NAT + word n-gram model: the finish loop with n-gram shallow fusion (include/cassnat_hip_nat_ngram.h)
    def nat_attach_ngram(self, desc, lm_scale=0.0):
        """``desc`` a ``CnNgramDesc`` over tables on this engine's device (copied; the caller keeps the tables alive while attached) is
        the model of this NAT engine's n-gram finish loop, ``lm_scale`` = float32(lm_weight * ln 10); None detaches."""
        self._chk(self.L.cn_nat_attach_ngram(self.handle, C.byref(desc) if desc is not None else None, float(lm_scale)),
                  "cn_nat_attach_ngram")

    def nat_ngram_finish(self, opts, ymax, beam_width, eos, length_penalty, zero_past_len, hyp, hyp_len, score):
        """The finish loop with the attached n-gram model after a pass that kept its rows (``opts.reserved[0] = 1``); the outputs are
        ``nat_lm_finish``'s."""
        self._chk(self.L.cn_nat_ngram_finish(self.handle, C.byref(opts), int(ymax), int(beam_width), int(eos),
                                             int(length_penalty is not None), float(length_penalty or 0.0), int(bool(zero_past_len)),
                                             _ptr(hyp), hyp.shape[2], _ptr(hyp_len), _ptr(score), current_stream()), "cn_nat_ngram_finish")

    def lm_step_begin(self, max_len, max_slots):
        self._chk(self.L.cn_lm_step_begin(self.handle, int(max_len), int(max_slots)), "cn_lm_step_begin")

    def lm_step(self, pos, tok, anc, keyok, logp):
        self._chk(self.L.cn_lm_step(self.handle, tok.shape[0], pos, _ptr(tok), _ptr(anc), _ptr(keyok), anc.shape[1], _ptr(logp),
                                current_stream()), "cn_lm_step")

    def ast_ctc_score(self, out_len, utt, last_tok, cand, prev_ref, parity, eos, score):
        self._chk(self.L.cn_ast_ctc_score(self.handle, cand.shape[0], out_len, _ptr(utt), _ptr(last_tok), _ptr(cand), cand.shape[1],
                                      _ptr(prev_ref), parity, eos, _ptr(score), current_stream()), "cn_ast_ctc_score")

    # ---- ESA sampling + LM ranking
    def esa_begin(self, feats, opts):
        B, T, F = feats.shape
        self._chk(self.L.cn_esa_begin(self.handle, _ptr(feats), B, T, F, C.byref(opts), current_stream()), "cn_esa_begin")

    def esa_sample(self, select, threshold, size_ratio, opts, tok, val, ylen, force_U=0):
        """One pass over n sampled alignments per utterance (n <= cfg.esa_group): select uint8 (n, B, T') cuda draws (all-zero
        = the best path) -> rows (U) of this pass; tok / val (n, B, stride), ylen (n, B).  force_U > 0: decode on that many
        rows; force_U = -1: only count the rows (tok / val / ylen may be None)."""
        ymax = C.c_int32()
        n = select.shape[0]
        assert select.is_contiguous()
        if force_U >= 0 and opts.beam_width == 1:  # (beam_width > 1: the per-row top-k stays in the engine, nothing is copied out)
            assert tok.shape[0] == n and tok.is_contiguous() and val.is_contiguous() and ylen.is_contiguous()
        self._chk(self.L.cn_esa_sample(self.handle, _ptr(select), n, float(threshold), _ptr(size_ratio), C.byref(opts), _ptr(tok),
                                   _ptr(val), tok.shape[2] if tok is not None else 0, _ptr(ylen), C.byref(ymax), int(force_U),
                                   current_stream()), "cn_esa_sample")
        return ymax.value

    def lm_score(self, tok, tgt, length, U, score):
        """tok / tgt int32 (N, ld), length int32 (N,), score float32 (N, ld): log p(tgt[n][u] | tok[n][..u]) for u < U."""
        self._chk(self.L.cn_lm_score(self.handle, _ptr(tok), _ptr(tgt), _ptr(length), tok.shape[0], int(U), tok.shape[1], _ptr(score),
                                 current_stream()), "cn_lm_score")

    def ast_decode(self, feats, opts, ast_opts, hyp, hyp_len, score):
        """Whole beam search on the device: hyp int32 (B, beam, max_len), hyp_len int32 (B, beam), score float64 (B, beam)."""
        B, T, F = feats.shape
        self._chk(self.L.cn_decode_ast(self.handle, _ptr(feats), B, T, F, C.byref(opts), C.byref(ast_opts), _ptr(hyp),
                                   hyp.shape[2], _ptr(hyp_len), _ptr(score), current_stream()), "cn_decode_ast")

    # ---- decode_type ctc_only / ctc_att, rank_model at_baseline
    def _ctc_search(self, name, head, feats, size_ratio, opts, beam, pruning, length_penalty, mid=(), with_lm=True, tail=()):
        """The call of a CTC prefix beam search entry ``name`` with freshly allocated outputs: ``head`` goes behind the handle, ``mid``
        behind the length penalty, ``tail`` behind nbeam -> (hyp, hyp_len, score_ctc, [score_lm,] p_blk, p_nblk, nbeam)."""
        import torch

        B, T, F = feats.shape
        cap = subsampled(T) + 1
        dev = feats.device
        hyp = torch.empty(B, beam, cap, dtype=torch.int32, device=dev)
        hlen = torch.empty(B, beam, dtype=torch.int32, device=dev)
        scores = [torch.empty(B, beam, dtype=torch.float64, device=dev) for _ in range(4 if with_lm else 3)]  # score_ctc, [score_lm,] p_blk, p_nblk
        nb = torch.empty(B, dtype=torch.int32, device=dev)
        self._chk(getattr(self.L, name)(self.handle, *head, _ptr(feats), _ptr(size_ratio), B, T, F, C.byref(opts), int(beam), int(pruning),
                                        float(length_penalty), *mid, _ptr(hyp), cap, _ptr(hlen), *(_ptr(t) for t in scores), _ptr(nb), *tail,
                                        current_stream()), name)
        return (hyp, hlen, *scores, nb)

    def ctc_beam(self, feats, size_ratio, opts, beam, pruning, length_penalty):
        """CTC prefix beam search on the device -> (hyp (B, beam, T'+1) int32, hyp_len (B, beam) int32, score_ctc / p_blk /
        p_nblk (B, beam) float64, nbeam (B,) int32) as cuda tensors; hypotheses carry no sos, best first."""
        return self._ctc_search("cn_ctc_beam", (), feats, size_ratio, opts, beam, pruning, length_penalty, with_lm=False)

    def ctc_beam_lm(self, lm, feats, size_ratio, opts, beam, pruning, length_penalty, lm_weight):
        """CTC prefix beam search with the TransformerLM engine ``lm`` (same library) in the frame loop (``cn_ctc_beam_lm``) ->
        ``ctc_beam``'s tuple with score_lm (B, beam) float64 behind score_ctc, and the loop's iteration count last."""
        if lm is None or lm.L is not self.L:
            raise HipError("cn_ctc_beam_lm: the LM engine comes from the other library")
        iters = C.c_int32()
        out = self._ctc_search("cn_ctc_beam_lm", (lm.handle,), feats, size_ratio, opts, beam, pruning, length_penalty, mid=(float(lm_weight),),
                               tail=(C.byref(iters),))
        return (*out, iters.value)

    def ctc_beam_ngram(self, desc, feats, size_ratio, opts, beam, pruning, length_penalty, lm_scale):
        """CTC prefix beam search with a word n-gram model in the frame loop (``cn_ctc_beam_ngram``): ``desc`` a ``CnNgramDesc`` over
        tables on the feats' device, ``lm_scale`` = ctc_lm_weight * ln(10) -> ``ctc_beam``'s tuple with score_lm (B, beam) float64
        behind score_ctc."""
        return self._ctc_search("cn_ctc_beam_ngram", (C.byref(desc),), feats, size_ratio, opts, beam, pruning, length_penalty, mid=(float(lm_scale),))

    def ctc_beam_bias(self, desc, feats, size_ratio, opts, beam, pruning, length_penalty):
        """CTC prefix beam search with contextual phrase biasing in the frame loop (``cn_ctc_beam_bias``): ``desc`` a ``CnBiasDesc``
        over tables on the feats' device (``models.bias.BiasList.desc``) -> ``ctc_beam_ngram``'s tuple, score_lm the banked bonus."""
        return self._ctc_search("cn_ctc_beam_bias", (C.byref(desc),), feats, size_ratio, opts, beam, pruning, length_penalty)

    def ctc_beam_merged(self, feats, size_ratio, opts, beam, pruning, length_penalty, ngram_desc=None, lm_scale=0.0, bias_desc=None):
        """CTC prefix beam search that merges candidates spelling the same prefix (``cn_ctc_beam_merged``;
        include/cassnat_hip_ctc_merge.h): without fusion, with ``ngram_desc`` (a ``CnNgramDesc``; ``lm_scale`` = ctc_lm_weight * ln(10))
        or with ``bias_desc`` (a ``CnBiasDesc``), at most one of the two -> ``ctc_beam_ngram``'s tuple (score_lm zeros without fusion)."""
        head = (C.byref(ngram_desc) if ngram_desc is not None else None, float(lm_scale), C.byref(bias_desc) if bias_desc is not None else None)
        return self._ctc_search("cn_ctc_beam_merged", head, feats, size_ratio, opts, beam, pruning, length_penalty)

    # ---- word / token time stamps: forced CTC alignment with spans and confidences (include/cassnat_hip_ctc_times.h)
    def ctc_token_times(self, feats, size_ratio, opts, labels, label_len):
        """Forced CTC alignment of ``labels`` (B, ld) int32 (no sos / eos / blank; ``label_len`` (B,) int32 of them count) on this
        engine's own log-posteriors of ``feats`` (``cn_ctc_token_times``: encoder + CTC head, then one launch) -> (start (B, ld) int32,
        end (B, ld) int32 exclusive, conf_lp (B, ld) float32, score (B,) float64, status (B,) int32) as cuda tensors, in subsampled
        frames; status 0 aligned, 1 no path, 2 a bad label.  ``size_ratio`` is not read (the valid frames are the key mask's)."""
        import torch

        B, T, F = feats.shape
        dev = feats.device
        labels = labels.to(dev, torch.int32).contiguous()
        label_len = label_len.to(dev, torch.int32).contiguous()
        ld = labels.shape[1]
        start = torch.full((B, ld), -1, dtype=torch.int32, device=dev)
        end = torch.full((B, ld), -1, dtype=torch.int32, device=dev)
        conf = torch.zeros(B, ld, dtype=torch.float32, device=dev)
        score = torch.empty(B, dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        self._chk(self.L.cn_ctc_token_times(self.handle, _ptr(feats), _ptr(size_ratio), B, T, F, C.byref(opts), _ptr(labels), ld, _ptr(label_len),
                                            _ptr(start), _ptr(end), _ptr(conf), _ptr(score), _ptr(status), current_stream()), "cn_ctc_token_times")
        return start, end, conf, score, status

    def lm_step_rows(self, max_pos, tok, pos, stay, rowid, logp):
        self._chk(self.L.cn_lm_step_rows(self.handle, tok.shape[0], int(max_pos), _ptr(tok), _ptr(pos), _ptr(stay), _ptr(rowid),
                                         rowid.shape[1], _ptr(logp), current_stream()), "cn_lm_step_rows")

    def decode_forced(self, feats, size_ratio, opts, labels, label_len, max_label_len, hyp, hyp_len, score):
        B, T, F = feats.shape
        self._chk(self.L.cn_decode_nast_forced(self.handle, _ptr(feats), _ptr(size_ratio), B, T, F, C.byref(opts), _ptr(labels),
                                           _ptr(label_len), labels.shape[1], int(max_label_len), _ptr(hyp), hyp.shape[1],
                                           _ptr(hyp_len), _ptr(score), current_stream()), "cn_decode_nast_forced")

    def ast_teacher_score(self, feats, opts, tok, tgt, length, n_per_utt, U, score):
        B, T, F = feats.shape
        self._chk(self.L.cn_ast_teacher_score(self.handle, _ptr(feats), B, T, F, C.byref(opts), _ptr(tok), _ptr(tgt), _ptr(length),
                                          int(n_per_utt), int(U), tok.shape[1], _ptr(score), current_stream()), "cn_ast_teacher_score")

    def ast_ctc_correct(self, feats, opts, k):
        """Transformer.fast_decode_with_ctc's device half: -> (length (B,) int32 cuda, tok (B, U, k) int32 cuda, val (B, U, k) f32 cuda)."""
        import torch

        B, T, F = feats.shape
        Tp = subsampled(T)
        tok = torch.empty(B * (Tp + 1) * k, dtype=torch.int32, device=feats.device)
        val = torch.empty(B * (Tp + 1) * k, dtype=torch.float32, device=feats.device)
        length = torch.empty(B, dtype=torch.int32, device=feats.device)
        rows = C.c_int32()
        self._chk(self.L.cn_ast_ctc_correct(self.handle, _ptr(feats), B, T, F, C.byref(opts), int(k), _ptr(tok), _ptr(val), _ptr(length),
                                        C.byref(rows), current_stream()), "cn_ast_ctc_correct")
        U = rows.value
        return length, tok[: B * U * k].view(B, U, k), val[: B * U * k].view(B, U, k)

    def profile_begin(self, tags=None):
        """Start HIP-event timing of the tagged kernels (None = all) on the launch stream."""
        self._chk(self.L.cn_profile_begin(self.handle, None if not tags else "|".join(tags).encode()), "cn_profile_begin")

    def profile_end(self):
        """-> {tag: {count, ms, flops, bytes}} accumulated since profile_begin (synchronises the device)."""
        import json

        buf = C.create_string_buffer(1 << 16)
        self._chk(self.L.cn_profile_end(self.handle, buf, len(buf)), "cn_profile_end")
        return json.loads(buf.value.decode())

    def shape(self, name):
        """Shape of a tensor ``fetch`` would return, without copying it (``shape("tok")[1]``: the row count of the last pass)."""
        shape = (C.c_int64 * 4)()
        ndim, dtype = C.c_int32(), C.c_int32()
        self._chk(self.L.cn_fetch(self.handle, name.encode(), None, 0, shape, C.byref(ndim), C.byref(dtype)), f"shape {name}")
        return tuple(shape[i] for i in range(ndim.value))

    def fetch(self, name):
        shape = (C.c_int64 * 4)()
        ndim, dtype = C.c_int32(), C.c_int32()
        self._chk(self.L.cn_fetch(self.handle, name.encode(), None, 0, shape, C.byref(ndim), C.byref(dtype)), f"fetch {name}")
        out = np.empty([shape[i] for i in range(ndim.value)], dtype=DTYPES[dtype.value])
        self._chk(self.L.cn_fetch(self.handle, name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes, shape,
                              C.byref(ndim), C.byref(dtype)), f"fetch {name}")
        return out
