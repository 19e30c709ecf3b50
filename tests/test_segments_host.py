"""Kaldi segments on the audio path, host side: the reader and its arithmetic (data/segments.py), the dataset's slices from one
memory map per recording, the CTM writer with offsets, bin/make_segments on its host leg end to end, and the refusals.  No GPU."""
import mmap
import os
from types import SimpleNamespace

import numpy as np
import pytest

import segments_cases as S
from cassnat_asr_public_amd.bin import make_fbank as mf
from cassnat_asr_public_amd.bin import make_segments as ms
from cassnat_asr_public_amd.data import kaldi_io, segments
from cassnat_asr_public_amd.data.speech_loader import SpeechDataset
from cassnat_asr_public_amd.utils import ctm


def test_the_sample_range():
    assert segments.sample_of(0.00003125, 16000) == 1 and segments.sample_of(0.00009375, 16000) == 2  # x.5 rounds up: floor(x + 0.5)
    assert segments.sample_of(0.0000312, 16000) == 0 and segments.sample_of(1.0005, 16000) == 16008
    assert segments.sample_range(0.5, 1.25, 16000, 32000) == (8000, 20000)
    assert segments.sample_range(0.5, -1, 16000, 32000) == (8000, 32000)  # END = -1: the end of the recording
    assert segments.sample_range(1.0, 2.49, 16000, 32000) == (16000, 32000)  # 0.49 s beyond the file: cut
    assert segments.sample_range(0.0, 2.0 + 0.5, 16000, 32000) == (0, 32000)
    with pytest.raises(ValueError, match="segment u1 of recording r1.*beyond"):
        segments.sample_range(1.0, 2.51, 16000, 32000, "u1", "r1")
    with pytest.raises(ValueError, match="segment u1 of recording r1.*negative"):
        segments.sample_range(-0.1, 1.0, 16000, 32000, "u1", "r1")
    for start, end in ((1.0, 1.0), (1.5, 1.0), (2.0, -1), (1.0, -2)):
        with pytest.raises(ValueError, match="segment u1 of recording r1.*empty or inverted"):
            segments.sample_range(start, end, 16000, 32000, "u1", "r1")
    # a time printed with three decimals names the sample it was computed from (truncation would lose one here)
    for k in (4641, 16008, 7777777):
        assert segments.sample_of(float("%.3f" % (k * 160 / 16000)), 16000) == k * 160


def test_the_reader(tmp_path):
    f = tmp_path / "segments"
    f.write_text("u1 r1 0 1.5\n\nu2 r1 1.25 -1\nu3 r2 0.5 0.75\n")
    assert segments.read_segments(str(f)) == [("u1", "r1", 0.0, 1.5), ("u2", "r1", 1.25, -1.0), ("u3", "r2", 0.5, 0.75)]
    for text, word in (("u1 r1 0 1.5 A\n", "fifth field"), ("u1 r1 0\n", "UTT REC START END"), ("u1 r1 0 x\n", "numbers"),
                       ("u1 r1 0 1\nu1 r1 1 2\n", "duplicate"), ("", "no segment"), ("u1 r1 0 inf\n", "finite")):
        f.write_text(text)
        with pytest.raises(ValueError, match=word):
            segments.read_segments(str(f))
    with pytest.raises(ValueError, match="segment u3 of recording r9.*unknown"):
        segments.check_recordings([("u1", "r1", 0, 1), ("u3", "r9", 0, 1)], ["r1", "r2"])


def dataset(scp, seg, conf="", **kw):
    args = SimpleNamespace(left_ctx=0, right_ctx=0, skip_frame=1, rank=0, hip_fbank_conf=conf, hip_audio="auto", hip_segments=seg, **kw)
    return SpeechDataset(None, [{"name": "t", "scp_path": scp}], args)


def two_recordings(tmp_path):
    x = S.recording()
    st = S.stereo_441(x)
    S.write_wave(tmp_path / "mono.wav", x)
    S.write_wave(tmp_path / "st.wav", st, 44100, 2)
    return x, st


def test_the_dataset_hands_out_the_bytes_of_the_range(tmp_path, monkeypatch):
    x, st = two_recordings(tmp_path)
    maps = []
    real = mmap.mmap
    monkeypatch.setattr(mmap, "mmap", lambda *a, **k: maps.append(1) or real(*a, **k))
    # mono at the front end's rate: the plain int16 pass
    S.write_wave(tmp_path / "mono2.wav", x)
    (tmp_path / "wav.scp").write_text("recA %s\nrecB %s\n" % (tmp_path / "mono.wav", tmp_path / "mono2.wav"))
    (tmp_path / "segments").write_text("a2 recA 1.0 2.00003125\na1 recA 0.5 1.5\nb1 recB 4.5 -1\na3 recA 4.9 5.4\n")
    ds = dataset(str(tmp_path / "wav.scp"), str(tmp_path / "segments"))
    assert ds.is_wave and ds.wave_plain and [it[0] for it in ds._items] == ["a2", "a1", "b1", "a3"]
    want = [(16000, 32001), (8000, 24000), (72000, 80200), (78400, 80200)]
    assert ds.wave_ranges == want and ds.wave_frames == [1 + (b - a - 400) // 160 for a, b in want]
    assert ds.segment_offsets == {"a2": ("recA", 1.0), "a1": ("recA", 0.5), "b1": ("recB", 4.5), "a3": ("recA", 4.9)}
    for k in (0, 1, 2, 3, 1, 0):
        utt, view, _ = ds[k]
        a, b = want[k]
        assert view.dtype == np.dtype("<i2") and view.flags.c_contiguous and view.tobytes() == x[a:b].tobytes()
    assert len(maps) == 2 and len(ds._maps) == 2  # one memory map per recording, however many segments it carries
    # a 44.1 kHz stereo recording: the interleaved slice [first * 2, last * 2), the frames those of the resampled wave
    conf = tmp_path / "fbank.conf"
    conf.write_text("--allow-downsample=true\n--channel=1\n")
    (tmp_path / "wav.scp").write_text("recS %s\n" % (tmp_path / "st.wav"))
    (tmp_path / "segments").write_text("s1 recS 0.25 1.0\ns2 recS 0.00001134 0.5\n")
    ds = dataset(str(tmp_path / "wav.scp"), str(tmp_path / "segments"), str(conf))
    assert not ds.wave_plain and ds.wave_formats == [(44100, 2)] * 2 and ds.wave_ranges == [(11025, 44100), (1, 22050)]
    from cassnat_asr_public_amd import hip

    assert ds.wave_frames == [1 + (hip.resample_num_samples(44100, 16000, b - a) - 400) // 160 for a, b in ds.wave_ranges]
    for k, (a, b) in enumerate(ds.wave_ranges):
        assert ds[k][1].tobytes() == st[2 * a:2 * b].tobytes()
    assert len(maps) == 3
    # without the flag nothing changes: one item per line, no ranges
    plain = dataset(str(tmp_path / "wav.scp"), "", str(conf))
    assert plain.wave_ranges is None and plain.segment_offsets is None and len(plain) == 1 and plain[0][1].tobytes() == st.tobytes()


def test_bad_segments_are_errors_before_anything_is_decoded(tmp_path):
    two_recordings(tmp_path)
    scp, seg = tmp_path / "wav.scp", tmp_path / "segments"
    scp.write_text("recA %s\n" % (tmp_path / "mono.wav"))
    for text, word in (("u1 recA 4.0 5.6\n", "segment u1 of recording recA.*beyond"), ("u1 recA -1 2\n", "segment u1 of recording recA.*negative"),
                       ("u1 recA 2 2\n", "segment u1 of recording recA.*empty"), ("u1 recA 3 2\n", "segment u1 of recording recA.*inverted"),
                       ("u1 recZ 0 1\n", "segment u1 of recording recZ.*unknown"), ("u1 recA 0 1\nu1 recA 1 2\n", "segment u1 of recording recA.*duplicate"),
                       ("u1 recA 0 1 0\n", "segment u1.*fifth field"), ("u0 recA 0 1\nu1 recA 1.0 1.0249\n", "segment u1 of recording recA.*no frame")):
        seg.write_text(text)
        with pytest.raises(ValueError, match=word):
            dataset(str(scp), str(seg))
    seg.write_text("u1 recA 4.0 5.5\n")  # 0.4875 s beyond the 5.0125 s: cut to the file
    assert dataset(str(scp), str(seg)).wave_ranges == [(64000, 80200)]


def test_flac_and_feature_sets_are_refused(tmp_path):
    seg = tmp_path / "segments"
    seg.write_text("u1 recA 0 1\n")
    (tmp_path / "a.flac").write_bytes(b"fLaC" + bytes(64))
    (tmp_path / "flac.scp").write_text("recA %s\n" % (tmp_path / "a.flac"))
    with pytest.raises(ValueError, match="hip_segments.*FLAC"):
        dataset(str(tmp_path / "flac.scp"), str(seg))
    kaldi_io.write_ark_scp(str(tmp_path / "f.ark"), str(tmp_path / "feats.scp"), [("recA", np.zeros((5, 4), np.float32))])
    with pytest.raises(ValueError, match="hip_segments.*not audio"):
        dataset(str(tmp_path / "feats.scp"), str(seg))
    with pytest.raises(ValueError, match="hip_segments.*not audio"):
        mf.make_fbank(str(tmp_path / "feats.scp"), str(tmp_path / "o"), segments=str(seg))
    with pytest.raises(ValueError, match="FLAC"):
        ms.make_segments(str(tmp_path / "flac.scp"), str(tmp_path / "o"), hip_vad="host")
    assert not os.path.exists(tmp_path / "o")
    from cassnat_asr_public_amd.utils.parser import DecodeParser

    assert DecodeParser().get_args(["--hip_segments", "x"]).hip_segments == "x" and DecodeParser().get_args([]).hip_segments == ""


RECORD = (["▁a", "b", "▁c"], [2, 5, 9], [5, 8, 12], [-0.1, -0.5, -0.2], 0, 20)


def test_the_ctm_writer_with_offsets(tmp_path):
    today = ["u1 1 0.08 0.24 ab 0.607", "u1 1 0.36 0.12 c 0.819"]
    assert ctm.lines("u1", RECORD, 0.04, "word") == today
    assert ctm.lines("u1", RECORD, 0.04, "word", ("recA", 12.345)) == ["recA 1 12.43 0.24 ab 0.607", "recA 1 12.71 0.12 c 0.819"]
    bad = RECORD[:4] + (1, 20)  # not aligned: the units share the frames evenly
    assert ctm.lines("u2", bad, 0.04, "word", ("recA", 100.0)) == ["recA 1 100.00 0.40 ab 0.000", "recA 1 100.40 0.40 c 0.000"]
    records = {"u1": RECORD, "u2": bad}
    assert ctm.write(str(tmp_path / "a.ctm"), ["u1", "u2"], records, 0.04, "word") == 1
    assert open(tmp_path / "a.ctm").read() == "\n".join(today + ["u2 1 0.00 0.40 ab 0.000", "u2 1 0.40 0.40 c 0.000"]) + "\n"
    assert ctm.write(str(tmp_path / "b.ctm"), ["u1", "u2"], records, 0.04, "word", offsets={"u1": ("recA", 12.345), "u2": ("recB", 0.5)}) == 1
    assert open(tmp_path / "b.ctm").read() == ("recA 1 12.43 0.24 ab 0.607\nrecA 1 12.71 0.12 c 0.819\n"
                                               "recB 1 0.50 0.40 ab 0.000\nrecB 1 0.90 0.40 c 0.000\n")


def test_make_segments_on_the_host_leg(tmp_path, capsys):
    """The recording of tests/vad_model.py: speech at the samples [8000, 38000), [42000, 51000) and [52200, 68200), so at 400 / 160 the
    frames that touch speech are [48, 238), [261, 319) and [324, 427).  Defaults (gaps of 23 and 5 frames are shorter than 30, pad 10):
    frames [38, 437) = 0.380 s to (436 * 160 + 400) / 16000 = 4.385 s.  With --min_silence 0.05 --pad 0.02 the three runs stay apart."""
    x, _ = two_recordings(tmp_path)
    S.write_wave(tmp_path / "quiet.wav", np.random.RandomState(3).randint(-3, 4, 20000).astype("<i2"))
    S.write_wave(tmp_path / "tiny.wav", x[:100])
    scp = tmp_path / "wav.scp"
    scp.write_text("recA %s\nquiet %s\ntiny %s\n" % (tmp_path / "mono.wav", tmp_path / "quiet.wav", tmp_path / "tiny.wav"))
    out = str(tmp_path / "out")
    c = ms.make_segments(str(scp), out, hip_vad="host")
    assert open(os.path.join(out, "segments")).read() == "recA-00000380-00004385 recA 0.380 4.385\n"
    assert c == {"recordings": 3, "frames": 499 + 123, "passes": 1, "segments": 1, "silent": 2}
    err = capsys.readouterr().err
    assert "quiet" in err and "tiny" in err and "recA" not in err
    assert sorted(os.listdir(out)) == sorted(ms.NAMES)
    table = dict(kaldi_io.read_scp(os.path.join(out, "vad.scp")))
    ark = open(os.path.join(out, "vad.ark"), "rb").read()
    at = int(table["recA"].rpartition(":")[2])
    assert ark[at:at + 6] == b"\0BFV \x04" and np.frombuffer(ark[at + 6:at + 10], "<i4")[0] == 499
    dec = np.frombuffer(ark[at + 10:at + 10 + 4 * 499], "<f4")
    assert set(dec) == {0.0, 1.0} and dec[48:238].all() and not dec[238:261].any() and dec[261:319].all() and dec[324:427].all() and dec.sum() == 190 + 58 + 103
    # several rows and passes per recording write the same files
    for chunk, cap in ((100, ms.PASS_BYTES), (100, 70000), (7, 5000)):
        again = str(tmp_path / "again")
        c2 = ms.make_segments(str(scp), again, hip_vad="host", chunk_frames=chunk, pass_bytes=cap)
        assert c2["passes"] >= (1 if cap == ms.PASS_BYTES else 3)
        assert open(os.path.join(again, "segments")).read() == open(os.path.join(out, "segments")).read()
        assert open(os.path.join(again, "vad.ark"), "rb").read() == ark
    c = ms.make_segments(str(scp), out, hip_vad="host", min_silence=0.05, pad=0.02)
    assert open(os.path.join(out, "segments")).read() == ("recA-00000460-00002415 recA 0.460 2.415\nrecA-00002590-00003225 recA 2.590 3.225\n"
                                                          "recA-00003220-00004305 recA 3.220 4.305\n")
    # the file it writes is a file the reader takes
    (tmp_path / "one.scp").write_text("recA %s\n" % (tmp_path / "mono.wav"))
    ds = dataset(str(tmp_path / "one.scp"), os.path.join(out, "segments"))
    assert ds.wave_ranges == [(7360, 38640), (41440, 51600), (51520, 68880)]
    # --max_segment 2 (200 frames): the run [38, 437) is cut at the lowest frame of [138, 238) - frame 237, which holds 80 samples of
    # speech and 320 of noise - and the rest, 200 frames, stays whole
    c = ms.make_segments(str(scp), out, hip_vad="host", max_segment=2.0)
    assert open(os.path.join(out, "segments")).read() == "recA-00000380-00002385 recA 0.380 2.385\nrecA-00002370-00004385 recA 2.370 4.385\n"


def test_a_pass_is_closed_at_its_row_limit_and_a_chunk_beyond_int32_is_refused(tmp_path):
    x, _ = two_recordings(tmp_path)
    scp = tmp_path / "wav.scp"
    scp.write_text("recA %s\nrecB %s\n" % (tmp_path / "mono.wav", tmp_path / "mono.wav"))
    recs = ms.open_recordings(str(scp), 25.0, 10.0, -1)
    passes, places, cap = ms.plan_passes(recs, 7, pass_rows=50)
    assert [len(p) for p in passes] == [50, 50, 44] and sum(c.frames for p in passes for c in p) == 2 * 499 and cap == 2 * 499
    assert ms.PASS_ROWS == 65535
    out, again = str(tmp_path / "out"), str(tmp_path / "again")
    ms.make_segments(str(scp), out, hip_vad="host")
    ms.make_segments(str(scp), again, hip_vad="host", chunk_frames=7, pass_rows=50)
    assert open(os.path.join(out, "segments")).read() == open(os.path.join(again, "segments")).read()
    assert open(os.path.join(out, "vad.ark"), "rb").read() == open(os.path.join(again, "vad.ark"), "rb").read()
    huge = [ms.Recording("big", "big.wav", 2 ** 31, 16000, 1, 400, 160, 1 + (2 ** 31 - 400) // 160)]
    with pytest.raises(ValueError, match="big.*int32.*chunk_frames"):
        ms.plan_passes(huge, 2 ** 30)
    assert len(ms.plan_passes(huge, 60000)[0]) > 1


def test_the_dataset_keeps_a_bounded_number_of_maps(tmp_path, monkeypatch):
    from cassnat_asr_public_amd.data import speech_loader

    x, _ = two_recordings(tmp_path)
    lines, segs = [], []
    for k in range(4):
        S.write_wave(tmp_path / ("r%d.wav" % k), x[:20000 + k])
        lines.append("r%d %s\n" % (k, tmp_path / ("r%d.wav" % k)))
        segs.append("u%d r%d 0.5 1.0\n" % (k, k))
    (tmp_path / "wav.scp").write_text("".join(lines))
    (tmp_path / "segments").write_text("".join(segs))
    monkeypatch.setattr(speech_loader, "MAX_SEGMENT_MAPS", 2)
    ds = dataset(str(tmp_path / "wav.scp"), str(tmp_path / "segments"))
    views = [ds[k][1] for k in (0, 1, 0, 2, 3, 0)]
    assert len(ds._maps) == 2 and all(v.tobytes() == x[8000:16000].tobytes() for v in views)  # (a view outlives its map's place in the table)


def test_make_segments_refusals(tmp_path):
    x, _ = two_recordings(tmp_path)
    S.write_wave(tmp_path / "hi.wav", x[:96000 // 2], 96000)
    scp = tmp_path / "wav.scp"
    scp.write_text("rec96 %s\n" % (tmp_path / "hi.wav"))
    with pytest.raises(ValueError, match="rec96.*2400 samples.*2048"):
        ms.make_segments(str(scp), str(tmp_path / "o"), hip_vad="host")
    scp.write_text("recS %s\n" % (tmp_path / "st.wav"))
    with pytest.raises(ValueError, match="recS.*--channel"):
        ms.make_segments(str(scp), str(tmp_path / "o"), hip_vad="host")
    conf = tmp_path / "vad.conf"
    conf.write_text("--vad-energy-threshold=4\n--snip-edges=true\n")
    scp.write_text("recA %s\n" % (tmp_path / "mono.wav"))
    with pytest.raises(ValueError, match="--snip-edges"):
        ms.make_segments(str(scp), str(tmp_path / "o"), vad_conf=str(conf), hip_vad="host")
    with pytest.raises(ValueError, match="hip_vad"):
        ms.make_segments(str(scp), str(tmp_path / "o"), hip_vad="cpu")
    assert not os.path.exists(tmp_path / "o")
    assert ms.main(["--data_path", str(scp), "--out_dir", str(tmp_path / "o"), "--hip_vad", "host"]) == 0
    assert open(tmp_path / "o" / "segments").read() == "recA-00000380-00004385 recA 0.380 4.385\n"
