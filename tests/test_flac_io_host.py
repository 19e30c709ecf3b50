"""FLAC input, host side: which `wav.scp` entries are FLAC entries (data/flac_io.py), the metadata chain and its refusals, the FLAC
set of the dataset against its WAV twin, and the exact frame index (cn_host_flac_index) against the frame offsets the model of the
tests wrote.  No GPU: the library's host entry points load without one."""
import numpy as np
import pytest
import torch

import flac_cases as fc
import flac_model as fm
from test_wave_io_host import data_args, fmt_chunk, riff, scp_of
from cassnat_asr_public_amd import hip
from cassnat_asr_public_amd.data import flac_io, kaldi_io, wave_io
from cassnat_asr_public_amd.data.speech_loader import FlacFrames, SpeechDataLoader, SpeechDataset, WaveBatch
from cassnat_asr_public_amd.pipeline import PackedBatch


def write_flac(path, pcm, bs=576, rate=16000, **kw):
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    data, first, offsets, _ = fm.write_stream(fm.simple_frames(pcm, bs, assignment=10 if pcm.shape[1] == 2 else None), rate=rate, **kw)
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def write_wav_twin(path, pcm, rate=16000):
    pcm = np.asarray(pcm).reshape(len(pcm), -1)
    return riff(path, [fmt_chunk(channels=pcm.shape[1], rate=rate)], pcm.astype("<i2").tobytes())


def index_of(data, first, rate=16000, channels=1):
    return hip.flac_index(np.frombuffer(data, np.uint8)[first:], rate, channels)


# ------------------------------------------------------------------------------------------------- entries
def test_entry_recognition(tmp_path):
    f = write_flac(tmp_path / "a b.flac", fc.walk(700, 1, seed=1))
    quoted = "'%s'" % f
    for spec in (f, "flac -c -d -s %s |" % quoted, "flac -cds %s |" % quoted, "flac -dc %s|" % quoted, "/usr/bin/flac --decode --stdout --silent %s |" % quoted,
                 "flac -s %s -d -c |" % quoted, "  flac -c -d %s |  " % quoted):
        assert flac_io.is_flac(spec) and flac_io.flac_path(spec) == f, spec
        assert wave_io.check_spec(spec, "u") == spec.strip() and not wave_io.is_wav(spec)
    wav = write_wav_twin(tmp_path / "a.wav", fc.walk(700, 1, seed=1))
    refused = ["sox %s -t wav - |" % quoted, "flac -c -d -s %s %s |" % (quoted, quoted), "flac -c -s %s |" % quoted, "flac -d -s %s |" % quoted,
               "flac -c -d -s --force %s |" % quoted, "flac -cdx %s |" % quoted, "flac -c -d -s |", "flac -c -d -s %s |" % (tmp_path / "missing.flac"),
               "flac -c -d -s %s |" % wav, "cat %s | flac -c -d -s - |" % quoted, "flac -c -d -s '%s |" % f]
    for spec in refused:
        assert not flac_io.is_flac(spec), spec
        with pytest.raises(ValueError, match="command") as e:
            wave_io.check_spec(spec, "spk-utt7")
        assert "spk-utt7" in str(e.value) and "no subprocess" in str(e.value)
    assert not flac_io.is_flac(wav) and not flac_io.is_flac(str(tmp_path / "missing.flac")) and not flac_io.is_flac(f + ":12")


# ------------------------------------------------------------------------------------------------- metadata
def test_metadata_walk_and_refusals(tmp_path):
    pcm = fc.walk(1000, 1, seed=2)
    seek = b"\xff\xf8\xc9\x18\x00\xc2" * 9  # a SEEKTABLE whose bytes hold sync patterns
    f = write_flac(tmp_path / "meta.flac", pcm, blocks=[(4, b"\x04\0\0\0test\0\0\0\0"), (3, seek), (1, bytes(37))])
    info = flac_io.read_info(f, "u")
    assert (info.rate, info.channels, info.bits, info.total) == (16000, 1, 16, 1000) and info.audio_offset == 4 + 38 + 4 + 12 + 4 + 54 + 4 + 37
    ix = flac_io.frame_index(f, info, "u")
    assert ix.samples == 1000 and ix.frames.shape == (2, 3) and ix.frames[:, 2].tolist() == [0, 576]
    data = open(f, "rb").read()

    def refused(name, body, reason, **kw):
        p = tmp_path / name
        p.write_bytes(body)
        with pytest.raises(ValueError, match=reason) as e:
            info = flac_io.checked(str(p), 16000, "spk-bad", **kw)
            flac_io.frame_index(str(p), info, "spk-bad")
        assert "spk-bad" in str(e.value)

    refused("id3.flac", b"ID3\x04" + data, "ID3")
    refused("ogg.flac", b"OggS" + data, "Ogg")
    refused("cut.flac", data[:60], "truncated metadata")
    refused("cut2.flac", data[:5], "truncated metadata")
    refused("nolast.flac", data[:4] + bytes([data[4] & 0x7F]) + data[5:42], "truncated metadata")
    frames = fm.simple_frames(pcm, 576)
    for bits in (8, 24):
        refused("b%d.flac" % bits, fm.write_stream(frames, bits=bits)[0], "%d-bit" % bits)
    refused("rate0.flac", fm.write_stream(frames, streaminfo_rate=0)[0], "sample rate 0")
    # frames that differ from STREAMINFO: another rate, another channel count, another sample size
    other = [dict(fr, rate_code=4) for fr in frames]
    refused("r8k.flac", fm.write_stream(other, rate=16000)[0], "differ from STREAMINFO")
    refused("r8k_later.flac", fm.write_stream(frames[:1] + other[1:], rate=16000)[0], "differ from STREAMINFO")
    refused("ch.flac", fm.write_stream(frames, streaminfo_channels=2)[0], "differ from STREAMINFO", channel=0)
    refused("bits.flac", fm.write_stream([dict(fr, size_code=6) for fr in frames])[0], "differ from STREAMINFO")
    # the admission rules of the WAV path
    refused("hi.flac", fm.write_stream(frames, rate=44100)[0], "allow-downsample")
    refused("lo.flac", fm.write_stream(frames, rate=8000)[0], "allow-upsample")
    st = fm.write_stream(fm.simple_frames(fc.walk(1000, 2, seed=3), 576))[0]
    refused("st.flac", st, "channels")
    refused("st5.flac", st, "--channel=5", channel=5)


# ------------------------------------------------------------------------------------------------- the dataset
def test_flac_set_equals_its_wav_twin(tmp_path):
    counts = [400, 559, 560, 6935, 4097]
    flacs, wavs = [], []
    for i, n in enumerate(counts):
        pcm = fc.walk(n, 1, seed=10 + i)
        f = write_flac(tmp_path / ("u%d.flac" % i), pcm, bs=[576, 192, 4096, 1152, 4096][i], total=0 if i == 3 else None)
        flacs.append(("u%d" % i, f if i % 2 else "flac -c -d -s %s |" % f))
        wavs.append(("u%d" % i, write_wav_twin(tmp_path / ("u%d.wav" % i), pcm)))
    ds = SpeechDataset(None, scp_of(tmp_path, flacs, "flac.scp"), data_args())
    tw = SpeechDataset(None, scp_of(tmp_path, wavs, "wav.scp"), data_args())
    assert ds.is_wave and ds.is_flac and ds.matrix_kinds() == frozenset(["FLAC"]) and ds.can_defer_cmvn() and not tw.is_flac
    assert ds.wave_frames == tw.wave_frames == [1, 1, 2, 41, 24] and ds.wave_formats == tw.wave_formats  # (#3: STREAMINFO total 0, from the index)
    utt, got, text = ds[3]
    assert utt == "u3" and isinstance(got, FlacFrames) and got.view.dtype == np.uint8 and not got.view.flags.writeable and text == [1]
    assert got.index.samples == 6935 and got.index.frames.dtype == np.int32 and got.index.frames[:, 2].tolist() == list(range(0, 6935, 1152))
    assert int(got.index.frames[-1, 0] + got.index.frames[-1, 1]) == got.view.shape[0]
    np.testing.assert_array_equal(fm.read_stream(open(flacs[3][1], "rb").read())[0][:, 0], tw[3][1])
    assert SpeechDataset(None, scp_of(tmp_path, flacs, "flac.scp"), data_args(hip_audio="1")).is_flac
    assert not SpeechDataset(None, scp_of(tmp_path, flacs[1::2], "plain.scp"), data_args(hip_audio="0")).is_wave
    a = next(iter(SpeechDataLoader(ds, 3, padding_idx=0)))
    b = next(iter(SpeechDataLoader(tw, 3, padding_idx=0)))
    assert isinstance(a[1], WaveBatch) and a[1].shape == b[1].shape == (3, 2, 80) and a[1].frames == b[1].frames and a[0] == b[0]
    assert a[1].formats == [(16000, 1)] * 3 and [ix.samples for ix in a[1].index] == counts[:3] and b[1].index is None
    assert torch.equal(a[3], b[3]) and torch.equal(a[2], b[2])
    pb = PackedBatch.from_waves(a[1].views, a[1].frames, 80, utts=a[0], formats=a[1].formats, index=a[1].index)
    assert pb.kinds == "flac" and pb.shape == (3, 2, 80) and pb.index == a[1].index
    with pytest.raises(NotImplementedError, match="wave form"):
        pb.padded()
    with pytest.raises(ValueError, match="utterance u1"):
        PackedBatch.from_waves([a[1].views[0], a[1].views[1][:-1], a[1].views[2]], a[1].frames, 80, utts=a[0], formats=a[1].formats, index=a[1].index)
    with pytest.raises(NotImplementedError, match="left_ctx"):
        SpeechDataset(None, scp_of(tmp_path, flacs, "flac.scp"), data_args(left_ctx=1))
    # the admission options, and a set too short for a frame
    conf = tmp_path / "fbank.conf"
    conf.write_text("--allow-downsample=true\n--allow-upsample=true\n--channel=1\n")
    mixed = [("hi", write_flac(tmp_path / "hi.flac", fc.walk(4410, 2, seed=20), rate=44100)), ("lo", write_flac(tmp_path / "lo.flac", fc.walk(800, 1, seed=21), rate=8000))]
    mw = [("hi", write_wav_twin(tmp_path / "hi.wav", fc.walk(4410, 2, seed=20), 44100)), ("lo", write_wav_twin(tmp_path / "lo.wav", fc.walk(800, 1, seed=21), 8000))]
    dm = SpeechDataset(None, scp_of(tmp_path, mixed, "m.scp"), data_args(hip_fbank_conf=str(conf)))
    tm = SpeechDataset(None, scp_of(tmp_path, mw, "mw.scp"), data_args(hip_fbank_conf=str(conf)))
    assert dm.wave_frames == tm.wave_frames and dm.wave_formats == tm.wave_formats == [(44100, 2), (8000, 1)]
    with pytest.raises(ValueError, match="no frame") as e:
        SpeechDataset(None, scp_of(tmp_path, flacs + [("spk-short", write_flac(tmp_path / "s.flac", fc.walk(399, 1)))], "s.scp"), data_args())
    assert "spk-short" in str(e.value)


def test_set_level_mixes(tmp_path):
    f = write_flac(tmp_path / "a.flac", fc.walk(1600, 1, seed=1))
    w = write_wav_twin(tmp_path / "a.wav", fc.walk(1600, 1, seed=1))
    ark = str(tmp_path / "one.ark")
    kaldi_io.write_ark_scp(ark, str(tmp_path / "unused.scp"), [("spk-fm", np.zeros((5, 80), np.float32))])
    for other, what in ((("spk-wav", w), "WAV files"), (("spk-fm", ark), "feature matrices")):
        for order in (0, 1):
            entries = [("spk-flac", "flac -c -d -s %s |" % f), other][::1 - 2 * order]
            with pytest.raises(ValueError, match="mixes FLAC entries and " + what) as e:
                SpeechDataset(None, scp_of(tmp_path, entries), data_args())
            assert "spk-flac" in str(e.value) and other[0] in str(e.value)
    with pytest.raises(ValueError, match="command") as e:
        SpeechDataset(None, scp_of(tmp_path, [("spk-flac", f), ("spk-pipe", "flac -c -d -s %s |" % (tmp_path / "missing.flac"))]), data_args())
    assert "spk-pipe" in str(e.value)


# ------------------------------------------------------------------------------------------------- the index
@pytest.mark.parametrize("k", range(6))
def test_index_equals_the_models_offsets(k):
    u = fc.utterances()[k]  # fixed and variable block sizes, 1- and 2-byte block-size codes, last frames of 1, 5 and 15 samples
    frames, samples = index_of(u["data"], u["first"], channels=u["channels"])
    assert samples == len(u["pcm"]) and frames[:, 0].tolist() == u["offsets"]
    assert frames[:, 2].tolist() == [int(v) for v in np.cumsum([0] + u["sizes"][:-1])]
    assert (frames[:, 0] + frames[:, 1]).tolist() == u["offsets"][1:] + [len(u["data"]) - u["first"]]


@pytest.mark.parametrize("variable", [False, True])
def test_index_across_the_coded_number_boundary(variable):
    """130 frames of 16 samples (frame numbers 127 -> 128: one byte -> two; sample numbers 2032 -> 2048 -> 2064 likewise) and a
    final frame of ONE sample."""
    pcm = fc.walk(130 * 16 + 1, 1, seed=30)
    data, first, offsets, _ = fm.write_stream(fm.simple_frames(pcm, 16, order=1), variable=variable)
    frames, samples = index_of(data, first)
    assert samples == len(pcm) and frames.shape[0] == 131 and frames[:, 0].tolist() == offsets and frames[-1, 2] == 2080
    lens = np.diff(offsets)
    assert lens[128] > lens[126] or variable  # (the header grew by a byte at frame 128)


def test_a_whole_frame_header_inside_a_payload_is_stepped_over():
    """A verbatim subframe whose samples spell a complete frame header - sync, valid codes, the expected NEXT frame number, a correct
    CRC-8: a scanner that trusts headers splits the frame there, the index (CRC-16 of everything before) does not."""
    fake = fm.frame_header(1, 192, 0)
    assert len(fake) == 6 and fm.crc8(fake[:-1]) == fake[-1]
    pcm = fc.walk(192 * 3, 1, seed=31)
    pcm[20:23, 0] = np.frombuffer(fake, ">i2")  # (the verbatim samples are byte-aligned: the subframe header is 8 bits)
    frames = fm.simple_frames(pcm, 192)
    frames[0]["subframes"] = [dict(type="verbatim")]
    data, first, offsets, _ = fm.write_stream(frames)
    at = data.find(fake, first + 6)
    assert first + 6 < at < first + offsets[1]  # the fake header lies inside frame 0's payload ...
    got, samples = index_of(data, first)
    assert got[:, 0].tolist() == offsets and samples == 576  # ... and the index has three frames, not four


def test_the_librarys_crc16_is_the_models():
    rng = np.random.default_rng(40)
    for n in list(range(0, 40)) + [255, 256, 257, 4093, 65537]:
        data = rng.integers(0, 256, n).astype(np.uint8).tobytes()
        assert hip.flac_crc16(data) == fm.crc16(data), n
    assert hip.flac_crc16(b"123456789") == 0xFEE8


def test_index_refusals():
    pcm = fc.walk(192 * 4 + 7, 1, seed=32)
    data, first, offsets, _ = fm.write_stream(fm.simple_frames(pcm, 192))
    audio = np.frombuffer(data, np.uint8)[first:]
    assert hip.flac_index(audio, 16000, 1)[1] == len(pcm)
    # truncated: the chain breaks in the frame the cut falls into
    # (a cut that leaves less than a whole header of frame 4 leaves no frame 4: frame 3 is then the one that never ends)
    for cut, where in ((offsets[2] + 40, offsets[2]), (offsets[4] + 3, offsets[3]), (len(audio) - 1, offsets[4]), (5, 0)):
        with pytest.raises(hip.FlacIndexError, match="byte offset %d" % where) as e:
            hip.flac_index(np.ascontiguousarray(audio[:cut]), 16000, 1)
        assert e.value.code == -2 and e.value.offset == where and isinstance(e.value, ValueError)
    # single flipped bytes: in a payload, in a header, in a CRC-16 - the chain breaks at the frame that holds the byte (a flipped
    # header byte of frame k makes frame k - 1 endless: the break is reported there)
    for at, where in ((offsets[1] + 30, offsets[1]), (offsets[3] - 1, offsets[2]), (offsets[2] + 1, offsets[1]), (offsets[4] + 9, offsets[4]), (2, 0)):
        bad = audio.copy()
        bad[at] ^= 0x24
        with pytest.raises(hip.FlacIndexError, match="byte offset %d" % where) as e:
            hip.flac_index(bad, 16000, 1)
        assert e.value.offset == where
    with pytest.raises(hip.FlacIndexError, match="STREAMINFO") as e:
        hip.flac_index(audio, 16000, 2)  # (the frames' rate code says "as STREAMINFO", their channel code says one)
    assert e.value.code == -3 and e.value.offset == 0


def test_total_mismatch_and_unknown_total(tmp_path):
    pcm = fc.walk(1000, 1, seed=33)
    frames = fm.simple_frames(pcm, 192)
    p = tmp_path / "wrong.flac"
    p.write_bytes(fm.write_stream(frames, total=999)[0])
    info = flac_io.read_info(str(p), "spk-w")
    with pytest.raises(ValueError, match="1000 samples, STREAMINFO says 999") as e:
        flac_io.frame_index(str(p), info, "spk-w")
    assert "spk-w" in str(e.value)
    q = tmp_path / "unknown.flac"
    q.write_bytes(fm.write_stream(frames, total=0)[0])
    info = flac_io.read_info(str(q))
    assert info.total == 0 and flac_io.frame_index(str(q), info).samples == 1000 and flac_io.num_samples(str(q)) == 1000
    cut = tmp_path / "cut.flac"
    cut.write_bytes(q.read_bytes()[:-20])
    with pytest.raises(ValueError, match="byte offset") as e:
        SpeechDataset(None, scp_of(tmp_path, [("spk-cut", str(cut))]), data_args())
    assert "spk-cut" in str(e.value)
