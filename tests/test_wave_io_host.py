"""Audio input, host side: the RIFF/WAVE reader (data/wave_io.py), the wave-set dataset and its refusals, Fbank.from_conf and the
packed reader's wave form (PackedBatch.from_waves).  No GPU."""
import struct
import wave
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.data import kaldi_io, wave_io
from cassnat_asr_public_amd.data.fbank import Fbank
from cassnat_asr_public_amd.data.speech_loader import SpeechDataLoader, SpeechDataset, WaveBatch
from cassnat_asr_public_amd.pipeline import PackedBatch


def samples_of(n, seed=0):
    x = np.random.default_rng(seed).integers(-32768, 32768, size=n).astype("<i2")
    x[:4] = [-32768, 32767, -32768, 32767]
    return x


def fmt_chunk(tag=1, channels=1, rate=16000, bits=16, extensible_sub=None):
    body = struct.pack("<HHIIHH", 0xFFFE if extensible_sub is not None else tag, channels, rate, rate * channels * bits // 8,
                       channels * bits // 8, bits)
    if extensible_sub is not None:  # cbSize 22: valid bits, channel mask, sub-format GUID (its first two bytes are the format tag)
        body += struct.pack("<HHI", 22, bits, 0) + struct.pack("<H", extensible_sub) + bytes.fromhex("000000001000800000aa00389b71")
    return b"fmt " + struct.pack("<I", len(body)) + body


def riff(path, chunks, data, data_size=None):
    """A RIFF/WAVE file of the given chunks (bytes, already framed) followed by the data chunk."""
    body = b"WAVE" + b"".join(chunks) + b"data" + struct.pack("<I", len(data) if data_size is None else data_size) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body) & 0xFFFFFFFF) + body)
    return str(path)


def stdlib_samples(path):
    with wave.open(path, "rb") as w:
        return np.frombuffer(w.readframes(w.getnframes()), "<i2")


def test_plain_header_written_by_the_stdlib(tmp_path):
    x = samples_of(1601)
    path = str(tmp_path / "a.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1), w.setsampwidth(2), w.setframerate(16000)
        w.writeframes(x.tobytes())
    assert wave_io.read_header(path) == (16000, 1, 16, 1, 44, 2 * 1601)
    v = wave_io.pcm_view(path, 16000)
    assert v.dtype == np.dtype("<i2") and not v.flags.writeable and v.base is not None  # (a view into the map, no copy)
    np.testing.assert_array_equal(v, stdlib_samples(path))
    np.testing.assert_array_equal(v, x)
    assert v.min() == -32768 and v.max() == 32767
    assert wave_io.num_samples(path, 16000) == 1601 and wave_io.is_wav(path)


@pytest.mark.parametrize("case", ["list", "odd", "extensible", "streamed", "zero_size"])
def test_chunks_before_data_and_streamed_sizes(tmp_path, case):
    x = samples_of(777, 3)
    path = tmp_path / (case + ".wav")
    if case == "list":
        riff(path, [fmt_chunk(), b"LIST" + struct.pack("<I", 12) + b"INFOabcdefgh", b"fact" + struct.pack("<II", 4, 777)], x.tobytes())
    elif case == "odd":  # a chunk of 5 bytes carries a pad byte: `data` starts at an even position
        riff(path, [fmt_chunk(), b"note" + struct.pack("<I", 5) + b"hello" + b"\0"], x.tobytes())
    elif case == "extensible":
        riff(path, [fmt_chunk(extensible_sub=1)], x.tobytes())
    elif case == "streamed":
        riff(path, [fmt_chunk()], x.tobytes(), data_size=0xFFFFFFFF)
    else:
        riff(path, [fmt_chunk()], x.tobytes(), data_size=0)
    path = str(path)
    rate, channels, bits, tag, start, nbytes = wave_io.read_header(path)
    assert (rate, channels, bits, tag, nbytes) == (16000, 1, 16, 1, 2 * 777)
    v = wave_io.pcm_view(path, 16000, "utt1")
    np.testing.assert_array_equal(v, x)
    try:
        ref = stdlib_samples(path)
    except (wave.Error, EOFError):
        ref = None  # (the stdlib does not read every one of these)
    if ref is not None and case not in ("streamed", "zero_size"):
        np.testing.assert_array_equal(v, ref)
    assert wave_io.num_samples(path) == 777


@pytest.mark.parametrize("what,reason", [("stereo", "channels"), ("8k", "8000"), ("8bit", "8-bit"), ("float", "float"), ("long", "data chunk")])
def test_refused_files_name_the_utterance(tmp_path, what, reason):
    path = tmp_path / "bad.wav"
    x = samples_of(800, 5).tobytes()
    if what == "stereo":
        riff(path, [fmt_chunk(channels=2)], x)
    elif what == "8k":
        riff(path, [fmt_chunk(rate=8000)], x)
    elif what == "8bit":
        riff(path, [fmt_chunk(bits=8)], x)
    elif what == "float":
        riff(path, [fmt_chunk(tag=3, bits=32)], x)
    else:
        riff(path, [fmt_chunk()], x, data_size=len(x) + 2)
    for fn in (wave_io.pcm_view, wave_io.num_samples):
        with pytest.raises(ValueError, match=reason) as e:
            fn(str(path), 16000, "spk-utt7")
        assert "spk-utt7" in str(e.value)


def test_pipe_and_offset_entries_are_refused(tmp_path):
    with pytest.raises(ValueError, match="command") as e:
        wave_io.check_spec("sox a.flac -t wav - |", "spk-utt1")
    assert "spk-utt1" in str(e.value)
    with pytest.raises(ValueError, match=":offset") as e:
        wave_io.check_spec("a.wav:17", "spk-utt2")
    assert "spk-utt2" in str(e.value)
    assert not wave_io.is_wav("sox a.flac -t wav - |")


# ------------------------------------------------------------------------------------------------- dataset
def write_wav(path, n, seed=0):
    return riff(path, [fmt_chunk()], samples_of(n, seed).tobytes())


def data_args(**kw):
    a = SimpleNamespace(left_ctx=0, right_ctx=0, skip_frame=1, rank=1, hip_audio="auto", hip_fbank_conf="")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def scp_of(tmp_path, entries, name="wav.scp"):
    p = tmp_path / name
    p.write_text("".join("%s %s\n" % e for e in entries))
    return [{"name": "test", "scp_path": str(p)}]


def test_wave_set_hands_out_views_and_collates_a_wave_batch(tmp_path):
    counts = [400, 559, 560, 6935]
    paths = scp_of(tmp_path, [("u%d" % i, write_wav(tmp_path / ("u%d.wav" % i), n, i)) for i, n in enumerate(counts)])
    ds = SpeechDataset(None, paths, data_args())
    assert ds.is_wave and ds.matrix_kinds() == frozenset(["WAV"]) and ds.can_defer_cmvn()
    assert ds.wave_frames == [1, 1, 2, 41] and ds.num_mel == 80
    utt, view, text = ds[3]
    assert utt == "u3" and view.dtype == np.dtype("<i2") and view.shape == (6935,) and text == [1]
    np.testing.assert_array_equal(view, samples_of(6935, 3))
    loader = SpeechDataLoader(ds, 3, padding_idx=0)
    assert len(loader) == 2
    utts, feats, texts, ratios, sizes = next(iter(loader))
    assert isinstance(feats, WaveBatch) and feats.shape == (3, 2, 80) and feats.frames == [1, 1, 2] and utts == ["u0", "u1", "u2"]
    assert torch.equal(ratios, torch.tensor([1 / 2, 1 / 2, 2 / 2], dtype=torch.float32))
    # --hip_audio 0 never looks: the entries stay feature matrices
    assert not SpeechDataset(None, paths, data_args(hip_audio="0")).is_wave


def test_wave_set_refusals(tmp_path):
    good = write_wav(tmp_path / "good.wav", 1600)
    short = write_wav(tmp_path / "short.wav", 399)
    with pytest.raises(ValueError, match="no frame") as e:
        SpeechDataset(None, scp_of(tmp_path, [("spk-a", good), ("spk-short", short)]), data_args())
    assert "spk-short" in str(e.value)
    fm = str(tmp_path / "one.ark")
    kaldi_io.write_ark_scp(fm, str(tmp_path / "unused.scp"), [("spk-fm", np.zeros((5, 80), np.float32))])
    with pytest.raises(ValueError, match="mixes") as e:
        SpeechDataset(None, scp_of(tmp_path, [("spk-a", good), ("spk-fm", fm)]), data_args())
    assert "spk-fm" in str(e.value)
    with pytest.raises(NotImplementedError, match="left_ctx"):
        SpeechDataset(None, scp_of(tmp_path, [("spk-a", good)]), data_args(left_ctx=1))
    with pytest.raises(ValueError, match="command") as e:
        SpeechDataset(None, scp_of(tmp_path, [("spk-a", good), ("spk-pipe", "flac -d -c x.flac |")]), data_args())
    assert "spk-pipe" in str(e.value)
    with pytest.raises(ValueError, match=":offset") as e:
        SpeechDataset(None, scp_of(tmp_path, [("spk-off", good + ":44")]), data_args())
    assert "spk-off" in str(e.value)
    stereo = riff(tmp_path / "stereo.wav", [fmt_chunk(channels=2)], samples_of(3200).tobytes())
    with pytest.raises(ValueError, match="channels") as e:
        SpeechDataset(None, scp_of(tmp_path, [("spk-a", good), ("spk-st", stereo)]), data_args())
    assert "spk-st" in str(e.value)
    with pytest.raises(ValueError, match="hip_audio 1"):
        SpeechDataset(None, scp_of(tmp_path, [("spk-fm", fm)]), data_args(hip_audio="1"))


def test_auto_keeps_a_plain_path_feature_scp_on_the_archive_path(tmp_path):
    fm = str(tmp_path / "one.ark")
    kaldi_io.write_ark_scp(fm, str(tmp_path / "unused.scp"), [("spk-fm", np.ones((5, 80), np.float32))])
    assert not wave_io.is_wav(fm)
    ds = SpeechDataset(None, scp_of(tmp_path, [("spk-fm", fm)]), data_args(hip_audio="auto"))
    assert not ds.is_wave and ds.matrix_kinds() == frozenset(["FM"])
    assert ds[0][1].shape == (5, 80)


# ------------------------------------------------------------------------------------------------- front-end options
def default_block():
    o = hip.CnFbankOpts()
    hip.lib().cn_fbank_default_opts(o)
    return bytes(o)


def test_from_conf_reads_the_recipe_file(tmp_path):
    conf = tmp_path / "fbank.conf"
    conf.write_text("--window-type=hamming # the recipe's four options\n\n--sample-frequency=16000\n--num-mel-bins=80\n--use-energy=false\n")
    fb = Fbank.from_conf(str(conf))
    assert fb.key() == default_block() and [fb.num_frames(n) for n in (399, 400, 559, 560, 6935)] == [0, 1, 1, 2, 41]
    conf.write_text("# another front-end\n--window-type=povey\n--num-mel-bins=40\n--low-freq=60\n--high-freq=-400\n--frame-length=20\n"
                    "--frame-shift=5\n--preemphasis-coefficient=0.9\n--remove-dc-offset=false\n--use-power=false\n--use-log-fbank=true\n"
                    "--dither=0\n--snip-edges=true\n")
    o = Fbank.from_conf(str(conf)).o
    assert (o.window_type, o.num_mel, o.low_freq, o.high_freq, o.frame_length_ms, o.frame_shift_ms) == (1, 40, 60.0, -400.0, 20.0, 5.0)
    assert (o.remove_dc, o.use_power, o.use_log) == (0, 0, 1) and abs(o.preemph - 0.9) < 1e-7


@pytest.mark.parametrize("line,exc", [("--dither=1.0", NotImplementedError), ("--use-energy=true", NotImplementedError),
                                      ("--snip-edges=false", NotImplementedError), ("--vtln-low=100", ValueError)])
def test_from_conf_refuses(tmp_path, line, exc):
    conf = tmp_path / "fbank.conf"
    conf.write_text("--num-mel-bins=80\n" + line + "\n")
    with pytest.raises(exc):
        Fbank.from_conf(str(conf))


# ------------------------------------------------------------------------------------------------- packed reader, wave form
def test_packed_batch_from_waves():
    counts = [400, 559, 560, 6935]
    fb = Fbank()
    views = [samples_of(n, n) for n in counts]
    frames = [fb.num_frames(n) for n in counts]
    pb = PackedBatch.from_waves(views, frames, 80, utts=["a", "b", "c", "d"])
    assert pb.kinds == "wave" and pb.lens == [1, 1, 2, 41] and pb.shape == (4, 41, 80)
    assert torch.equal(pb.ratios(), torch.tensor([n / 41 for n in (1, 1, 2, 41)], dtype=torch.float32))
    with pytest.raises(NotImplementedError):
        pb.padded()
    with pytest.raises(NotImplementedError):
        pb.matrices()
    with pytest.raises(ValueError, match="utterance b"):
        PackedBatch.from_waves([views[0], views[1].astype(np.float32)], frames[:2], 80, utts=["a", "b"])
    with pytest.raises(ValueError, match="utterance short"):
        PackedBatch.from_waves([views[0], samples_of(399)], [1, fb.num_frames(399)], 80, utts=["a", "short"])
    with pytest.raises(ValueError, match="utterance #1"):
        PackedBatch.from_waves([views[0], views[3][::2]], [1, 20], 80)


def test_pipelines_refuse_the_wave_form_without_a_gpu_and_mixed_passes():
    from cassnat_asr_public_amd.pipeline import DecodePipelines

    pipes = DecodePipelines.__new__(DecodePipelines)
    pipes._on_gpu, pipes._device, pipes.cmvn = False, None, None
    wave_pb = PackedBatch.from_waves([samples_of(800)], [3], 80)
    rows_pb = PackedBatch([np.zeros((3, 80), np.float32)])
    with pytest.raises(NotImplementedError, match="wave form"):
        pipes._stage_packed(0, 0, [(wave_pb, wave_pb.ratios(), 0)], 0.0)
    with pytest.raises(ValueError, match="mixes wave"):
        pipes._stage_packed(0, 0, [(wave_pb, wave_pb.ratios(), 0), (rows_pb, rows_pb.ratios(), 1)], 0.0)
