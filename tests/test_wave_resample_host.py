"""Audio at other sample rates and channels, host side: cn_resample_num_samples and cn_resample_table against the float64 model
(tests/resample_model.py), the three Kaldi options in a conf file, the header checks of data/wave_io.py with them, the wave-set
dataset over a mixed wav.scp and the packed reader's wave form with (rate, channels).  No GPU."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import resample_model as rm
from test_wave_io_host import fmt_chunk, riff, samples_of
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.data import wave_io
from cassnat_asr_public_amd.data.fbank import Fbank, parse_conf
from cassnat_asr_public_amd.data.speech_loader import SpeechDataLoader, SpeechDataset, WaveBatch, frames_of
from cassnat_asr_public_amd.pipeline import DecodePipelines, PackedBatch


# ------------------------------------------------------------------------------------------------- counts and tables
@pytest.mark.parametrize("fi,fo", rm.PAIRS)
def test_num_samples_is_the_models(fi, fo):
    L = hip.lib()
    assert [L.cn_resample_num_samples(fi, fo, n) for n in range(2001)] == [rm.num_samples(fi, fo, n) for n in range(2001)]
    assert L.cn_resample_num_samples(fi, fo, -1) == 0 and L.cn_resample_num_samples(0, fo, 5) == 0
    assert L.cn_resample_num_samples(fi, fo, 2 ** 40) == rm.num_samples(fi, fo, 2 ** 40)  # (64-bit throughout)


def ulps(a, b):
    """Distance in float32 steps."""
    ia, ib = (np.asarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(v < 0, -(v & 0x7FFFFFFF), v) for v in (ia, ib))
    return np.abs(ia - ib)


@pytest.mark.parametrize("fi,fo", rm.PAIRS)
def test_table_is_the_models_rounded_once(fi, fo):
    """Units, first indices and tap counts exactly; every weight within 1 ulp of float32(model weight) (the two evaluate the same
    double expression with the same libm: equality is expected, the ulp allows for expression order).  Tap-major, zero behind a
    phase's own taps."""
    t = hip.resample_table(fi, fo)
    in_unit, out_unit, first, weights = rm.table(fi, fo)
    assert (t["in_unit"], t["out_unit"]) == (in_unit, out_unit)
    assert t["first"].tolist() == first and t["taps"].tolist() == [len(w) for w in weights]
    assert t["max_taps"] == max(len(w) for w in weights) and t["weights"].shape == (t["max_taps"], out_unit)
    worst = 0
    for p, w in enumerate(weights):
        got = t["weights"][:, p]
        worst = max(worst, int(ulps(got[: len(w)], w.astype(np.float32)).max()))
        assert (got[len(w):] == 0).all()
    print("\n[%d -> %d] worst weight distance %d ulp" % (fi, fo, worst))
    assert worst <= 1


def test_table_of_equal_rates_and_refusals():
    t = hip.resample_table(16000, 16000)
    assert (t["in_unit"], t["out_unit"], t["max_taps"]) == (1, 1, 1) and t["first"].tolist() == [0] and t["weights"].tolist() == [[1.0]]
    L = hip.lib()
    iu, ou, mt = C.c_int32(), C.c_int32(), C.c_int32()
    sizes = (C.byref(iu), C.byref(ou), C.byref(mt))
    assert L.cn_resample_table(0, 16000, *sizes, None, None, None, 0) != 0 and b"positive" in L.cn_last_error()
    assert L.cn_resample_table(16000, 16000, None, *sizes[1:], None, None, None, 0) != 0
    # 15999 -> 16000 Hz: 16000 phases of 13 taps
    assert L.cn_resample_table(15999, 16000, *sizes, None, None, None, 0) != 0 and b"65536" in L.cn_last_error()
    # 1 MHz -> 16 kHz: 256 outputs need 16 000 input samples
    assert L.cn_resample_table(1000000, 16000, *sizes, None, None, None, 0) != 0 and b"LDS" in L.cn_last_error()
    # arrays that are too small
    first, taps, w = np.zeros(2, np.int32), np.zeros(2, np.int32), np.full(30, 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.cn_resample_table(8000, 16000, *sizes, p(first), p(taps), p(w), 25) != 0 and (w == 7.0).all()
    assert L.cn_resample_table(8000, 16000, *sizes, p(first), p(taps), p(w), 26) == 0 and (w[:26] != 7.0).all() and (w[26:] == 7.0).all()


# ------------------------------------------------------------------------------------------------- conf file
def test_parse_conf_takes_the_three_options(tmp_path):
    conf = tmp_path / "fbank.conf"
    conf.write_text("--num-mel-bins=40\n--allow-downsample=true\n--allow-upsample=false  # telephone\n--channel=1\n")
    assert parse_conf(str(conf)) == {"num_mel": 40, "allow_downsample": 1, "allow_upsample": 0, "channel": 1}
    fb = Fbank.from_conf(str(conf))
    assert (fb.allow_downsample, fb.allow_upsample, fb.channel) == (True, False, 1)
    assert fb.admit() == {"allow_downsample": True, "allow_upsample": False, "channel": 1}
    # not part of the option block: the key is that of the same options without them
    assert fb.key() == Fbank(num_mel=40).key()
    plain = Fbank()
    assert (plain.allow_downsample, plain.allow_upsample, plain.channel) == (False, False, -1)
    conf.write_text("--channel=x\n")
    with pytest.raises(ValueError, match="channel"):
        parse_conf(str(conf))
    conf.write_text("--allow-upsample=yes\n")
    with pytest.raises(ValueError, match="allow-upsample"):
        parse_conf(str(conf))


# ------------------------------------------------------------------------------------------------- headers
def wav(path, n, rate=16000, channels=1, seed=0):
    """A file of n sample frames; -> (path, the interleaved int16)."""
    x = samples_of(n * channels, seed)
    return riff(path, [fmt_chunk(rate=rate, channels=channels)], x.tobytes()), x


def test_rates_need_their_option(tmp_path):
    hi, xh = wav(tmp_path / "hi.wav", 480, rate=48000)
    lo, xl = wav(tmp_path / "lo.wav", 80, rate=8000)
    for fn in (wave_io.wave_format, wave_io.pcm_frames, wave_io.num_samples, wave_io.pcm_view):
        with pytest.raises(ValueError, match="48000.*--allow-downsample=true") as e:
            fn(hi, 16000, "spk-hi")
        assert "spk-hi" in str(e.value)
        with pytest.raises(ValueError, match="8000.*--allow-upsample=true") as e:
            fn(lo, 16000, "spk-lo")
        assert "spk-lo" in str(e.value)
    # the other option does not help
    with pytest.raises(ValueError, match="--allow-downsample=true"):
        wave_io.wave_format(hi, 16000, "spk-hi", allow_upsample=True)
    with pytest.raises(ValueError, match="--allow-upsample=true"):
        wave_io.wave_format(lo, 16000, "spk-lo", allow_downsample=True)
    assert wave_io.wave_format(hi, 16000, "spk-hi", allow_downsample=True) == (480, 48000, 1)
    assert wave_io.wave_format(lo, 16000, "spk-lo", allow_upsample=True) == (80, 8000, 1)
    v, rate, ch = wave_io.pcm_frames(lo, 16000, "spk-lo", allow_upsample=True)
    assert (rate, ch) == (8000, 1) and v.dtype == np.dtype("<i2") and not v.flags.writeable
    np.testing.assert_array_equal(v, xl)


def test_channels_need_a_channel(tmp_path):
    path, x = wav(tmp_path / "three.wav", 100, channels=3)
    for ch in (-1, 3, 7):
        with pytest.raises(ValueError, match="3 channels.*--channel=0 .. 2") as e:
            wave_io.wave_format(path, 16000, "spk-three", channel=ch)
        assert "spk-three" in str(e.value)
    for ch in (0, 1, 2):
        assert wave_io.wave_format(path, 16000, "spk-three", channel=ch) == (100, 16000, 3)
        v, rate, chans = wave_io.pcm_frames(path, 16000, "spk-three", channel=ch)
        assert (rate, chans) == (16000, 3) and v.shape == (300,)
        np.testing.assert_array_equal(v, x)  # (the interleaved chunk: the channel is picked on the device)
    # a trailing partial sample frame is not handed out
    odd = riff(tmp_path / "odd.wav", [fmt_chunk(channels=3)], x.tobytes()[:-2])
    assert wave_io.wave_format(odd, 16000, None, channel=0)[0] == 99 and wave_io.pcm_frames(odd, 16000, None, channel=0)[0].shape == (297,)
    # a mono file takes any --channel, as Kaldi's (channel 0 of one)
    mono, _ = wav(tmp_path / "mono.wav", 50)
    assert wave_io.wave_format(mono, 16000, None, channel=0) == (50, 16000, 1)


# ------------------------------------------------------------------------------------------------- dataset
def data_args(conf="", **kw):
    a = SimpleNamespace(left_ctx=0, right_ctx=0, skip_frame=1, rank=1, hip_audio="auto", hip_fbank_conf=str(conf))
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def scp_of(tmp_path, entries, name="wav.scp"):
    path = tmp_path / name
    path.write_text("".join("%s %s\n" % e for e in entries))
    return [{"name": "test", "scp_path": str(path)}]


def mixed_set(tmp_path):
    files = [("spk-16k", wav(tmp_path / "a.wav", 6935)), ("spk-8k", wav(tmp_path / "b.wav", 3000, rate=8000, seed=1)),
             ("spk-44k", wav(tmp_path / "c.wav", 20000, rate=44100, channels=2, seed=2))]
    conf = tmp_path / "fbank.conf"
    conf.write_text("--allow-downsample=true\n--allow-upsample=true\n--channel=1\n")
    return files, conf


def test_dataset_over_a_mixed_wav_scp(tmp_path):
    files, conf = mixed_set(tmp_path)
    paths = scp_of(tmp_path, [(u, p) for u, (p, _) in files])
    ds = SpeechDataset(None, paths, data_args(conf))
    counts = [6935, rm.num_samples(8000, 16000, 3000), rm.num_samples(44100, 16000, 20000)]
    assert counts == [6935, 6000, 7257]
    assert ds.is_wave and ds.wave_formats == [(16000, 1), (8000, 1), (44100, 2)] and not ds.wave_plain
    assert ds.wave_frames == [frames_of(ds.fbank_opts, n) for n in counts] == [41, 36, 43]
    assert ds.wave_admit == {"allow_downsample": True, "allow_upsample": True, "channel": 1}
    for i, (utt, (_, x)) in enumerate(files):  # the data chunks as the files hold them
        got = ds[i]
        assert got[0] == utt
        np.testing.assert_array_equal(got[1], x)
    utts, feats, _, ratios, _ = next(iter(SpeechDataLoader(ds, 3, padding_idx=0)))
    assert isinstance(feats, WaveBatch) and feats.formats == ds.wave_formats and feats.frames == ds.wave_frames and feats.shape == (3, 43, 80)
    np.testing.assert_array_equal(ratios.numpy(), np.array([n / 43 for n in ds.wave_frames], np.float32))
    # without the options the first file that needs one is refused by name, with the option
    with pytest.raises(ValueError, match="spk-8k.*--allow-upsample=true"):
        SpeechDataset(None, paths, data_args())
    conf.write_text("--allow-upsample=true\n--allow-downsample=true\n")
    with pytest.raises(ValueError, match="spk-44k.*--channel"):
        SpeechDataset(None, paths, data_args(conf))
    conf.write_text("--allow-upsample=true\n--channel=1\n")
    with pytest.raises(ValueError, match="spk-44k.*--allow-downsample=true"):
        SpeechDataset(None, paths, data_args(conf))
    # a set of plain files is what it was: sample views, no formats in the batch
    plain = SpeechDataset(None, scp_of(tmp_path, [("spk-16k", files[0][1][0])], "p.scp"), data_args(conf))
    assert plain.wave_plain and next(iter(SpeechDataLoader(plain, 1, padding_idx=0)))[1].formats is None


def test_a_resampled_count_one_short_of_a_window_is_refused(tmp_path):
    """48 kHz -> 16 kHz: 1197 samples give 399 at 16 kHz (no frame), 1198 give 400 (one)."""
    assert rm.num_samples(48000, 16000, 1197) == 399 and rm.num_samples(48000, 16000, 1198) == 400
    conf = tmp_path / "fbank.conf"
    conf.write_text("--allow-downsample=true\n")
    ok, _ = wav(tmp_path / "ok.wav", 1198, rate=48000)
    short, _ = wav(tmp_path / "short.wav", 1197, rate=48000)
    assert SpeechDataset(None, scp_of(tmp_path, [("spk-ok", ok)]), data_args(conf)).wave_frames == [1]
    with pytest.raises(ValueError, match="spk-short.*399 samples.*no frame"):
        SpeechDataset(None, scp_of(tmp_path, [("spk-ok", ok), ("spk-short", short)]), data_args(conf))


# ------------------------------------------------------------------------------------------------- the packed reader's wave form
def test_packed_batch_keeps_rate_and_channels(tmp_path):
    views = [samples_of(6935), samples_of(3000, 1), samples_of(40000, 2)]
    formats = [(16000, 1), (8000, 1), (44100, 2)]
    pb = PackedBatch.from_waves(views, [41, 36, 43], 80, utts=["a", "b", "c"], formats=formats, channel=1)
    assert pb.kinds == "wave" and pb.formats == formats and pb.channel == 1 and pb.shape == (3, 43, 80) and pb.lens == [41, 36, 43]
    assert PackedBatch.from_waves(views[:1], [41], 80).formats is None
    with pytest.raises(ValueError, match="utterance c"):  # stereo, no channel named
        PackedBatch.from_waves(views, [41, 36, 43], 80, utts=["a", "b", "c"], formats=formats)
    with pytest.raises(ValueError, match="utterance c"):  # an odd number of values for two channels
        PackedBatch.from_waves(views[:2] + [views[2][:-1]], [41, 36, 43], 80, utts=["a", "b", "c"], formats=formats, channel=0)
    with pytest.raises(ValueError, match="pairs"):
        PackedBatch.from_waves(views, [41, 36, 43], 80, formats=formats[:2], channel=1)
    with pytest.raises(NotImplementedError):
        pb.padded()


def test_the_cpu_rehearsal_of_the_wave_form_still_raises():
    pipes = DecodePipelines.__new__(DecodePipelines)
    pipes._on_gpu, pipes._device, pipes.cmvn = False, None, None
    pb = PackedBatch.from_waves([samples_of(1600, 3)], [3], 80, formats=[(32000, 2)], channel=0)
    with pytest.raises(NotImplementedError, match="wave form"):
        pipes._stage_packed(0, 0, [(pb, pb.ratios(), 0)], 0.0)
