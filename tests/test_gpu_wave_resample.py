"""Audio at other sample rates and channels on the device: cn_op_wave_resample (Kaldi's LinearResample + channel pick, csrc/resample.hip)
against the float64 model of tests/resample_model.py, cn_op_fbank_packed_f32 against cn_fbank bit for bit, Fbank.packed and the
decode pipelines on mixed passes, and decode_asr end to end from a wav.scp of 44.1 kHz stereo, 8 kHz and 16 kHz files against the
`FM ` archive of the same device features.

The staged bytes always lie inside a larger tensor filled with 0x7F (int16 32639) and the outputs in tensors filled with a
sentinel: a wrong index gives wrong values or a touched sentinel, not a fault."""
import numpy as np
import pytest
import torch

import resample_model as rm
from conftest import tiny_case
from test_gpu_spliced_reader import Runs, fm_archive, nat_conf, tiny240
from test_gpu_wave_reader import NAT_KEYS, OPTS, cmvn_stats, write_model
from test_wave_io_host import fmt_chunk, riff
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.data.fbank import Fbank

pytestmark = pytest.mark.gpu

RUN = 256        # outputs per workgroup of wave_resample_kernel
SENT = 7.0e9     # (no resampled int16 wave comes near it)
PAD = -1.5
LEAD, TAIL = 4096, 8192  # sentinel bytes in front of and behind the staged bytes
COMBOS = [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]  # (channels, channel)


def noise(n, seed):
    """int16 noise with runs at both ends of the range (when it is long enough to hold them)."""
    x = np.random.default_rng(seed).integers(-32768, 32768, size=n).astype("<i2")
    if n >= 2:
        x[:2] = [-32768, 32767]
    if n >= 120:
        x[20:50], x[70:100] = -32768, 32767
    return x


def interleave(x, channels, c, seed):
    """x as channel c of an interleaved chunk; the other channels hold other noise."""
    data = np.random.default_rng(1000 + seed).integers(-32768, 32768, size=(len(x), channels)).astype("<i2")
    data[:, c] = x
    return np.ascontiguousarray(data.reshape(-1))


def length_for(fi, fo, target):
    """The input length whose output count is ``target`` - or, where no length gives it (8 -> 16 kHz: every count is even), the
    nearest count on the far side of it."""
    in_unit, out_unit = rm.units(fi, fo)
    n = max(1, target * in_unit // out_unit - 2)
    while rm.num_samples(fi, fo, n) < target:
        n += 1
    if rm.num_samples(fi, fo, n) != target and target % RUN == RUN - 1:
        n -= 1  # (one below a multiple: stay below it)
    return n


def lengths_of(fi, fo):
    in_unit, out_unit = rm.units(fi, fo)
    taps = max(len(w) for w in rm.table(fi, fo)[3])
    whole = 3 * in_unit  # n * fo / fi is an integer: the `last -= 1` branch of the count
    assert (whole * fo) % fi == 0
    return [1, 2, taps, whole, whole + 1, length_for(fi, fo, RUN - 1), length_for(fi, fo, RUN), length_for(fi, fo, RUN + 1),
            length_for(fi, fo, 2 * RUN + 1), length_for(fi, fo, 3 * RUN - 40)]


class Staged:
    """Data chunks at 16-byte-aligned offsets behind ``lead`` bytes inside a larger 0x7F-filled tensor, gaps filled with 0x7F too, and a
    sentinel-filled float32 output with 8 floats between the utterances' slots."""

    def __init__(self, chunks, channels, channel, counts, lead=0, staged_bytes=None):
        U = len(chunks)
        offs, total = hip.gather_offsets([v.nbytes for v in chunks], 16)
        offs = offs.astype(np.int64) + lead
        total = int(total + lead) if staged_bytes is None else int(staged_bytes)
        end = max(int(o) + v.nbytes for o, v in zip(offs, chunks))
        host = np.full(LEAD + max(total, end) + TAIL, 0x7F, np.uint8)
        for o, v in zip(offs, chunks):
            host[LEAD + o:LEAD + o + v.nbytes] = v.view(np.uint8)
        self.big = torch.from_numpy(host).cuda()
        self.staged, self.total = self.big[LEAD:], total
        self.ch_h, self.c_h = np.asarray(channels, np.int32), np.asarray(channel, np.int32)
        self.per = [len(v) // ch for v, ch in zip(chunks, channels)]
        self.out_off = np.zeros(U, np.int64)
        np.cumsum([(n + 3) // 4 * 4 + 8 for n in counts[:-1]], out=self.out_off[1:])
        self.counts = list(counts)
        self.floats = int(self.out_off[-1]) + (counts[-1] + 3) // 4 * 4 + 64
        dev = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device="cuda")
        self.off_d, self.per_d, self.ch_d, self.c_d, self.oo_d = dev(offs), dev(self.per), dev(self.ch_h), dev(self.c_h), dev(self.out_off)
        self.wave = torch.full((self.floats,), SENT, dtype=torch.float32, device="cuda")

    def run(self, fi, fo, rows=None):
        rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32, device="cuda")
        sel = range(len(self.counts)) if rows is None else rows
        hip.wave_resample(fi, fo, self.staged, self.total, self.off_d, self.per_d, self.ch_d, self.c_d, self.ch_h, self.c_h, self.wave,
                          self.oo_d, max(1, max(self.counts[r] for r in sel)), rows=rows_d)
        torch.cuda.synchronize()
        return self.wave.cpu().numpy()

    def split(self, wave, only=None):
        """-> the utterances' outputs; every float outside the slots of ``only`` (default: all) must still be the sentinel."""
        only = range(len(self.counts)) if only is None else only
        mask = np.ones(wave.shape[0], bool)
        rows = {}
        for r in only:
            o, n = int(self.out_off[r]), self.counts[r]
            rows[r] = wave[o:o + n]
            mask[o:o + n] = False
        assert (wave[mask] == np.float32(SENT)).all(), "a float outside the utterances' outputs was written"
        return rows


_models = {}


def model_case(fi, fo):
    """Per rate pair: the target channel of every utterance, the model's outputs and its bound sums - computed once."""
    if (fi, fo) not in _models:
        xs = [noise(n, 7 * i + fi % 97) for i, n in enumerate(lengths_of(fi, fo))]
        _models[(fi, fo)] = (xs, [rm.resample(x, fi, fo) for x in xs])
    return _models[(fi, fo)]


def check_against_model(got, x, fi, fo, want=None):
    """|dev - model| <= (taps + 3) * 2^-24 * sum_j |w_j x_j| per output: float32 accumulation over `taps` terms, the products, the table
    rounding.  -> the worst error as a fraction of the bound."""
    y, s = rm.resample(x, fi, fo) if want is None else want
    assert got.shape == y.shape
    in_unit, out_unit, _, weights = rm.table(fi, fo)
    taps = np.array([len(weights[k % out_unit]) for k in range(len(y))])
    bound = (taps + 3) * 2.0 ** -24 * s
    err = np.abs(got.astype(np.float64) - y)
    assert (err <= bound).all(), "worst error / bound %.3g at output %d" % (np.max(err / np.maximum(bound, 1e-300)), int(np.argmax(err - bound)))
    return float(np.max(err / np.maximum(bound, 1e-300))) if len(y) else 0.0


# ------------------------------------------------------------------------------------------------- 1. the kernel against the model
@pytest.mark.parametrize("fi,fo", rm.PAIRS)
def test_resample_kernel_against_the_model(fi, fo):
    xs, want = model_case(fi, fo)
    counts = [rm.num_samples(fi, fo, len(x)) for x in xs]
    assert counts[3] * fi == len(xs[3]) * fo and RUN in counts and max(counts) > 2 * RUN and min(counts) >= 1
    worst, first = 0.0, None
    for ci, (C, c) in enumerate(COMBOS):
        st = Staged([interleave(x, C, c, i) for i, x in enumerate(xs)], [C] * len(xs), [c] * len(xs), counts)
        rows = st.split(st.run(fi, fo))
        for r, x in enumerate(xs):
            worst = max(worst, check_against_model(rows[r], x, fi, fo, want[r]))
        if first is None:
            first = rows
        else:  # the same samples in another channel layout: the same float32 sums
            for r in rows:
                np.testing.assert_array_equal(rows[r], first[r])
    print("\n[%d -> %d] %d utterances x %d channel layouts: worst error %.3f of the bound" % (fi, fo, len(xs), len(COMBOS), worst))
    # every utterance its own channel layout; the utterances in another order behind a 48-byte lead: the same rows bit for bit
    order = [7, 0, 9, 3, 1, 8, 2, 6, 5, 4]
    combos = [COMBOS[(3 * j) % len(COMBOS)] for j in range(len(order))]
    st = Staged([interleave(xs[i], C, c, 50 + i) for i, (C, c) in zip(order, combos)], [C for C, _ in combos], [c for _, c in combos],
                [counts[i] for i in order], lead=48)
    again = st.split(st.run(fi, fo))
    for j, i in enumerate(order):
        np.testing.assert_array_equal(again[j], first[i])
    # a row list: the other utterances' slots are not touched
    st = Staged([interleave(xs[i], C, c, 50 + i) for i, (C, c) in zip(order, combos)], [C for C, _ in combos], [c for _, c in combos],
                [counts[i] for i in order], lead=48)
    some = [8, 1, 4]
    part = st.split(st.run(fi, fo, rows=some), only=some)
    for j in some:
        np.testing.assert_array_equal(part[j], first[order[j]])


# ------------------------------------------------------------------------------------------------- 2. equal rates
def test_equal_rates_pick_the_channel_exactly():
    xs = [noise(n, 3 + n) for n in (1, 255, 256, 257, 700)]
    st = Staged([interleave(x, 2, 1, i) for i, x in enumerate(xs)], [2] * len(xs), [1] * len(xs), [len(x) for x in xs])
    rows = st.split(st.run(16000, 16000))
    for r, x in enumerate(xs):
        np.testing.assert_array_equal(rows[r], x.astype(np.float32))
    assert rows[4].min() == -32768.0 and rows[4].max() == 32767.0


# ------------------------------------------------------------------------------------------------- 3. cut at the staged end
@pytest.mark.parametrize("fi,fo,C,c", [(48000, 16000, 1, 0), (44100, 16000, 2, 1), (8000, 16000, 3, 2)])
def test_an_utterance_past_the_staged_end_is_cut(fi, fo, C, c):
    """Three utterances; staged_bytes ends inside the second (in the middle of a sample frame), the third starts behind it.  Their
    bytes are all there, inside the tensor - what is read is what lies inside [0, staged_bytes)."""
    xs = [noise(900, 1), noise(1500, 2), noise(600, 3)]
    chunks = [interleave(x, C, c, i) for i, x in enumerate(xs)]
    offs, _ = hip.gather_offsets([v.nbytes for v in chunks], 16)
    keep = 1001  # whole sample frames of the second utterance inside
    cut = int(offs[1]) + 2 * C * keep + (2 * C - 1)
    full = [rm.num_samples(fi, fo, len(x)) for x in xs]
    st = Staged(chunks, [C] * 3, [c] * 3, full, staged_bytes=cut)
    wave = st.run(fi, fo)
    st.counts = [full[0], rm.num_samples(fi, fo, keep), 0]
    rows = st.split(wave)
    check_against_model(rows[0], xs[0], fi, fo)
    check_against_model(rows[1], xs[1][:keep], fi, fo)
    assert st.counts[1] < full[1] and rows[2].size == 0


# ------------------------------------------------------------------------------------------------- 4. fbank from the float wave
COUNTS = [400, 559, 560, 6935]


def resampled_wave(counts=COUNTS, fi=48000):
    """A device-resampled float32 wave of the given sample counts (fi -> 16 kHz) -> (wave cuda, byte offsets, counts on the device,
    the utterances' values on the host)."""
    xs = [noise(length_for(fi, 16000, n), 11 + n) for n in counts]
    assert [rm.num_samples(fi, 16000, len(x)) for x in xs] == list(counts)
    st = Staged(xs, [1] * len(xs), [0] * len(xs), list(counts))
    rows = st.split(st.run(fi, 16000))
    dev = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32, device="cuda")
    return st.wave, dev(st.out_off * 4), dev(counts), [rows[r] for r in range(len(xs))]


@pytest.mark.parametrize("with_cmvn", [False, True])
@pytest.mark.parametrize("opts", OPTS, ids=["default", "povey40", "hanning20ms"])
def test_fbank_packed_f32_is_cn_fbank_on_the_resampled_wave(opts, with_cmvn):
    wave, off, ns, rows = resampled_wave()
    assert max(np.abs(r).max() for r in rows) > 32768.0  # (resampled values leave the int16 range: the wave stays float32)
    fb = Fbank(**opts)
    frames = [fb.num_frames(n) for n in COUNTS]
    T = max(frames) + 3
    plain = torch.full((len(COUNTS), T, fb.o.num_mel), 7.0, device="cuda")
    hip.fbank_packed_f32(fb.o, wave, 4 * wave.numel(), off, ns, plain, PAD)
    torch.cuda.synchronize()
    got = plain.cpu().numpy()
    if not with_cmvn:
        ref, _ = fb(rows)  # cn_fbank on the same float32 values
        ref = ref.cpu().numpy()
        for b, n in enumerate(frames):
            assert n >= 1
            np.testing.assert_array_equal(got[b, :n], ref[b, :n])
            assert (got[b, n:] == np.float32(PAD)).all()
        return
    rng = np.random.default_rng(11)
    F = fb.o.num_mel
    mean, std = torch.from_numpy(rng.standard_normal(F) * 3 + 12).cuda(), torch.from_numpy(rng.random(F) + 0.5).cuda()
    normed = torch.full((len(COUNTS), T, F), 7.0, device="cuda")
    hip.fbank_packed_f32(fb.o, wave, 4 * wave.numel(), off, ns, normed, PAD, mean, std)
    want = hip.cmvn_(plain.clone(), torch.tensor(frames, dtype=torch.int32, device="cuda"), mean, std)
    torch.cuda.synchronize()
    normed = normed.cpu().numpy()
    np.testing.assert_array_equal(normed, want.cpu().numpy())
    for b, n in enumerate(frames):
        assert (normed[b, n:] == np.float32(PAD)).all() and not (normed[b, :n] == got[b, :n]).all()


def test_fbank_packed_f32_cuts_at_the_end_of_the_wave():
    """wave_bytes ends inside the second utterance: its frames are those of the samples inside, the rest is padding."""
    wave, off, ns, rows = resampled_wave([560, 6935])
    fb = Fbank()
    inside = 1000
    out = torch.full((2, 45, 80), 7.0, device="cuda")
    hip.fbank_packed_f32(fb.o, wave, int(off[1]) + 4 * inside + 3, off, ns, out, PAD)
    torch.cuda.synchronize()
    ref, _ = fb([rows[0], rows[1][:inside]])
    n = fb.num_frames(inside)
    got, ref = out.cpu().numpy(), ref.cpu().numpy()
    np.testing.assert_array_equal(got[0, :2], ref[0, :2])
    np.testing.assert_array_equal(got[1, :n], ref[1, :n])
    assert (got[0, 2:] == np.float32(PAD)).all() and (got[1, n:] == np.float32(PAD)).all()


# ------------------------------------------------------------------------------------------------- 5. Fbank.packed
def mixed_files():
    """(data chunk, rate, channels) of a 16 kHz mono, an 8 kHz mono, a 44.1 kHz stereo and a 48 kHz three-channel utterance; channel 1
    is read where there are several."""
    specs = [(6935, 16000, 1), (3300, 8000, 1), (20000, 44100, 2), (21000, 48000, 3)]
    return [(interleave(noise(n, 31 + i), C, min(1, C - 1), 60 + i), rate, C) for i, (n, rate, C) in enumerate(specs)]


def by_hand(fb, chunk, rate, C, channel=1):
    """Features of one file from the two entries themselves: (1) then (4)."""
    n = rm.num_samples(rate, 16000, len(chunk) // C)
    st = Staged([chunk], [C], [channel if C > 1 else 0], [n])
    st.run(rate, 16000)
    T = fb.num_frames(n)
    out = torch.full((1, T, fb.o.num_mel), 7.0, device="cuda")
    one = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")
    hip.fbank_packed_f32(fb.o, st.wave, 4 * st.wave.numel(), one(0), one(n), out, PAD, fb.mean64, fb.std64)
    torch.cuda.synchronize()
    return out[0]


def test_packed_of_plain_files_is_todays_path():
    views = [noise(n, n) for n in (400, 559, 6935)]
    fb = Fbank(pad_value=PAD, allow_downsample=True, allow_upsample=True, channel=1)
    a, ra = fb.packed(views)
    b, rb = fb.packed(views, rates=[16000] * 3, channels=[1] * 3)
    # ... which is hip.fbank_packed on the staged int16
    offs, total = hip.gather_offsets([v.nbytes for v in views], 16)
    host = np.zeros(total, np.uint8)
    for o, v in zip(offs, views):
        host[int(o):int(o) + v.nbytes] = v.view(np.uint8)
    dev = lambda x: torch.tensor(np.asarray(x).astype(np.int64), dtype=torch.int32, device="cuda")
    c = torch.full(tuple(a.shape), 7.0, device="cuda")
    hip.fbank_packed(fb.o, torch.from_numpy(host).cuda(), total, dev(offs), dev([len(v) for v in views]), c, PAD)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(ra, rb) and fb.resampled_passes == 0


@pytest.mark.parametrize("splice", [None, (0, 2, 1)])
def test_packed_of_mixed_files_is_the_composition(splice):
    files = mixed_files()
    rng = np.random.default_rng(3)
    mean, std = rng.standard_normal(80) * 3 + 12, rng.random(80) + 0.5
    fb = Fbank(cmvn_mean=mean, cmvn_std=std, pad_value=PAD, splice=splice, channel=1)
    feats, ratios = fb.packed([f[0] for f in files], utts=["a", "b", "c", "d"], rates=[f[1] for f in files], channels=[f[2] for f in files])
    torch.cuda.synchronize()
    assert fb.resampled_passes == 1
    frames = [fb.num_frames(rm.num_samples(rate, 16000, len(chunk) // C)) for chunk, rate, C in files]
    assert frames == [41, 39, 43, 42]
    n_out = frames
    for b, (chunk, rate, C) in enumerate(files):
        want = by_hand(fb, chunk, rate, C)
        if splice is not None:
            one = lambda v: torch.tensor([v], dtype=torch.int32, device="cuda")
            out = torch.full((1, frames[b], 240), 7.0, device="cuda")
            hip.splice_rows(want.contiguous(), one(0), one(frames[b]), out, splice[0], splice[1], splice[2], PAD)
            torch.cuda.synchronize()
            want = out[0]
        assert torch.equal(feats[b, :n_out[b]], want), b
        assert (feats[b, n_out[b]:] == PAD).all()
    assert torch.equal(ratios, torch.tensor([n / max(n_out) for n in n_out], dtype=torch.float32))
    # several channels and no channel named: refused by name
    with pytest.raises(ValueError, match="utterance c.*--channel"):
        Fbank().packed([f[0] for f in files], utts=["a", "b", "c", "d"], rates=[f[1] for f in files], channels=[f[2] for f in files])


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_wave_resample_refusals_leave_the_output_alone():
    L = hip.lib()
    xs = [noise(300, 1), noise(500, 2)]
    st = Staged([interleave(x, 2, 1, i) for i, x in enumerate(xs)], [2, 2], [1, 1], [100, 167])
    p, s = hip._ptr, hip.current_stream()
    hp = lambda a: a.ctypes.data_as(hip.C.c_void_p)

    def refused(fi=48000, fo=16000, staged=p(st.staged), off=p(st.off_d), per=p(st.per_d), ch=p(st.ch_d), c=p(st.c_d), ch_h=hp(st.ch_h),
                c_h=hp(st.c_h), utts=2, rows_d=None, rows=2, max_out=167, wave=p(st.wave), oo=p(st.oo_d), text=None):
        rc = L.cn_op_wave_resample(fi, fo, staged, st.total, off, per, ch, c, ch_h, c_h, utts, rows_d, rows, max_out, wave, oo, s)
        err = L.cn_last_error()
        return rc != 0 and len(err) > 0 and (text is None or text in err)

    for name in ("staged", "off", "per", "ch", "c", "ch_h", "c_h", "wave", "oo"):
        assert refused(**{name: None}, text=b"null"), name
    assert refused(fi=0, text=b"positive") and refused(fo=-16000, text=b"positive")
    assert refused(utts=0) and refused(rows=0) and refused(rows=-1) and refused(max_out=0) and refused(rows=3)  # (no row list: rows <= utts)
    bad = np.array([1, 2], np.int32)
    assert refused(c_h=hp(bad), text=b"channel 2 of 2") and refused(c_h=hp(np.array([-1, 0], np.int32)), text=b"channel -1")
    assert refused(ch_h=hp(np.array([2, 0], np.int32)), text=b"utterance #1")
    assert refused(fi=15999, fo=16000, text=b"65536") and refused(fi=1000000, fo=16000, text=b"LDS")
    torch.cuda.synchronize()
    assert (st.wave == SENT).all()
    # ... and the same call, not refused, writes
    assert not refused()
    torch.cuda.synchronize()
    assert (st.wave != SENT).sum() == 100 + 167


# ------------------------------------------------------------------------------------------------- 7. the decode pipelines
def test_pipelines_stage_a_mixed_pass():
    """One pass of three batches - 16 kHz mono, then 8 kHz mono and 44.1 kHz stereo, then 48 kHz three channels - through
    DecodePipelines' own staging: every utterance's features are Fbank.packed's of that file alone."""
    from test_gpu_pipeline import build
    from cassnat_asr_public_amd import synth
    from cassnat_asr_public_amd.pipeline import DecodePipelines, PackedBatch

    args = synth.make_args("tiny")
    args.hip_max_batch, args.hip_max_frames = 4, 90
    model = build(args, synth.make_state(args, seed=0, gain=2.0), "fp32")
    files = mixed_files()
    rng = np.random.default_rng(3)
    cmvn = (rng.standard_normal(80) * 3 + 12, rng.random(80) + 0.5)
    fb = Fbank(cmvn_mean=cmvn[0], cmvn_std=cmvn[1], pad_value=PAD, channel=1)
    frames = [fb.num_frames(rm.num_samples(rate, 16000, len(chunk) // C)) for chunk, rate, C in files]

    def batch(idx, plain=False):
        return PackedBatch.from_waves([files[i][0] for i in idx], [frames[i] for i in idx], 80, utts=["u%d" % i for i in idx],
                                      formats=None if plain else [files[i][1:] for i in idx], channel=-1 if plain else 1)

    with DecodePipelines(model, 1, 4, 90, cmvn=cmvn, fbank=fb.o) as pipes:
        pipes._on_gpu, pipes._device = True, torch.cuda.current_device()  # (what the first decode() would set: no worker thread here)
        pbs = [batch([0], plain=True), batch([1, 2]), batch([3])]
        feats, ratios = pipes._stage_packed(0, 0, [(pb, pb.ratios(), j) for j, pb in enumerate(pbs)], PAD)
        torch.cuda.synchronize()
        assert tuple(feats.shape) == (4, 43, 80) and pipes.stats["wave_passes"] == 1 and pipes.stats["resampled_passes"] == 1
        for b, (chunk, rate, C) in enumerate(files):
            alone, _ = fb.packed([chunk], rates=[rate], channels=[C])
            torch.cuda.synchronize()
            assert torch.equal(feats[b, :frames[b]], alone[0]), b
            assert (feats[b, frames[b]:] == PAD).all()
        assert torch.equal(ratios.cpu(), torch.cat([pb.ratios() for pb in pbs]))
        # a pass of plain files stays the int16 pass
        pipes._stage_packed(0, 0, [(pbs[0], pbs[0].ratios(), 0)], PAD)
        torch.cuda.synchronize()
        assert pipes.stats["wave_passes"] == 2 and pipes.stats["resampled_passes"] == 1


# ------------------------------------------------------------------------------------------------- 8. end to end
def write_wav(path, chunk, rate, channels):
    return riff(path, [fmt_chunk(rate=rate, channels=channels)], np.ascontiguousarray(chunk, dtype="<i2").tobytes())


def mixed_twins(tmp_path, counts, **fbank_opts):
    """WAV files of about the given frame counts - 44.1 kHz stereo, 8 kHz mono and 16 kHz mono in turn - with the conf file that admits
    them, and the `FM ` archive of the (unspliced) features Fbank.packed computes from them."""
    kinds = [(44100, 2), (8000, 1), (16000, 1)]
    chunks, rates, chans, lines = [], [], [], []
    for b, n in enumerate(counts):
        rate, C = kinds[b % 3]
        samples = (400 + 160 * (n - 1) + (37 * b) % 160) * rate // 16000
        chunk = interleave(noise(samples, 20 + b), C, min(1, C - 1), 80 + b)
        chunks.append(chunk), rates.append(rate), chans.append(C)
        lines.append("spk-utt%02d %s\n" % (b, write_wav(tmp_path / ("utt%02d.wav" % b), chunk, rate, C)))
    wscp = tmp_path / "wav.scp"
    wscp.write_text("".join(lines))
    conf = tmp_path / "fbank.conf"
    conf.write_text("--allow-downsample=true\n--allow-upsample=true\n--channel=1\n")
    feats, ratios = Fbank(channel=1, **fbank_opts).packed(chunks, rates=rates, channels=chans)
    torch.cuda.synchronize()
    feats = feats.cpu().numpy()
    got = [round(float(r) * feats.shape[1]) for r in ratios]
    assert all(abs(g - n) <= 1 for g, n in zip(got, counts))
    mats = [feats[b, :n].copy() for b, n in enumerate(got)]
    return str(wscp), fm_archive(tmp_path, mats), mats, str(conf)


E2E_COUNTS = [61, 37, 50, 44, 58, 39, 47]


@pytest.mark.parametrize("with_cmvn,pipelines", [(False, 2), (True, 2), (True, 1), (False, 1)])
def test_decode_from_a_mixed_wav_scp(tmp_path, monkeypatch, with_cmvn, pipelines):
    args, state, _, _ = tiny_case()
    wscp, fscp, mats, conf = mixed_twins(tmp_path, E2E_COUNTS)
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, tmp_path, mats if with_cmvn else None))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    flags = ["--hip_pipelines", pipelines, "--hip_precision", "fp32", "--hip_fbank_conf", conf]
    wav, fm = run(wscp, *flags), run(fscp, *flags)
    assert [ln.split()[0] for ln in wav] == ["spk-utt%02d" % b for b in range(len(E2E_COUNTS))] and all(len(ln.split()) > 1 for ln in wav)
    assert wav == fm
    s = run.stats
    if pipelines > 1:
        assert s[0]["passes"] >= 1 and s[0]["wave_passes"] == s[0]["resampled_passes"] == s[0]["passes"], s
        assert s[1]["wave_passes"] == s[1]["resampled_passes"] == 0, s
    else:
        assert not s[0] and not s[1]


def test_decode_from_a_mixed_wav_scp_with_right_ctx_2(tmp_path, monkeypatch):
    args, state = tiny240()
    wscp, fscp, mats, conf = mixed_twins(tmp_path, E2E_COUNTS)
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args, tmp_path, mats))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    flags = ["--hip_precision", "fp32", "--hip_fbank_conf", conf]
    wav, fm = run(wscp, *flags), run(fscp, *flags)
    assert wav == fm and len(wav) == len(E2E_COUNTS) and all(len(ln.split()) > 1 for ln in wav)
    assert wav == run(wscp, "--hip_pipelines", 1, *flags)
    s = run.stats
    assert s[0]["wave_passes"] == s[0]["resampled_passes"] == s[0]["spliced_passes"] == s[0]["passes"] >= 1, s


def test_a_mixed_wav_scp_without_the_options_is_refused(tmp_path):
    from cassnat_asr_public_amd.bin import decode_asr

    args, state, _, _ = tiny_case()
    wscp, _, _, _ = mixed_twins(tmp_path, [40, 41, 42])
    ckpt, cfg = write_model(tmp_path, args, state, {k: getattr(args, k) for k in NAT_KEYS})
    with pytest.raises(ValueError, match="spk-utt00.*--channel"):
        decode_asr.main(["--task", "cassnat", "--test_config", cfg, "--data_path", wscp, "--resume_model", ckpt,
                         "--result_file", str(tmp_path / "r.txt")])
