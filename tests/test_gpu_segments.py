"""Kaldi segments on the device path, end to end: bin/make_segments' device leg against its host leg, decode_asr --hip_segments and
make_fbank --hip_segments against the same runs on separately written WAV files that hold exactly the samples [first, last), the chain
make_segments -> decode_asr --hip_segments, and --hip_ctm under segments."""
import os

import numpy as np
import pytest

import segments_cases as S
from conftest import ast_tiny_case, tiny_case
from test_gpu_spliced_reader import Runs, nat_conf, tiny240
from test_gpu_wave_reader import write_model
from test_make_fbank_host import read_dir
from cassnat_asr_public_amd.bin import make_fbank as mf
from cassnat_asr_public_amd.bin import make_segments as ms
from cassnat_asr_public_amd.data import segments

pytestmark = pytest.mark.gpu

# overlapping, out of order, one to the end of the recording; the starts are multiples of 10 ms except s-d's
SEGS = [("s-b", 0.7, 1.31), ("s-a", 0.0, 0.45), ("s-c", 1.0, -1), ("s-d", 0.20053, 0.9)]
SAMPLES = 30000


def segment_set(tmp_path, stereo=False):
    """One recording with SEGS -> (wav.scp, segments file, the wav.scp of the pre-cut files under the segments' ids, fbank conf)."""
    rate, channels = (44100, 2) if stereo else (16000, 1)
    n = SAMPLES * rate // 16000  # (1.875 s)
    x = S.speech(n, 40)
    data = S.stereo_441(x) if stereo else x
    S.write_wave(tmp_path / "rec.wav", data, rate, channels)
    (tmp_path / "wav.scp").write_text("recA %s\nunused %s\n" % (tmp_path / "rec.wav", tmp_path / "rec.wav"))
    (tmp_path / "segments").write_text("".join("%s recA %s %s\n" % s for s in SEGS))
    lines = []
    for utt, start, end in SEGS:
        first, last = segments.sample_range(start, end, rate, n)
        lines.append("%s %s\n" % (utt, S.write_wave(tmp_path / (utt + ".wav"), data[first * channels:last * channels], rate, channels)))
    (tmp_path / "cut.scp").write_text("".join(lines))
    conf = ""
    if stereo:
        (tmp_path / "fbank.conf").write_text("--allow-downsample=true\n--channel=1\n")
        conf = str(tmp_path / "fbank.conf")
    return str(tmp_path / "wav.scp"), str(tmp_path / "segments"), str(tmp_path / "cut.scp"), conf


def long_set(tmp_path, stereo=False):
    x = S.recording()
    if stereo:
        S.write_wave(tmp_path / "rec.wav", S.stereo_441(x), 44100, 2)
        (tmp_path / "fbank.conf").write_text("--allow-downsample=true\n--channel=1\n")
    else:
        S.write_wave(tmp_path / "rec.wav", x)
    S.write_wave(tmp_path / "more.wav", x[20000:70000])
    (tmp_path / "wav.scp").write_text("recA %s\nrecB %s\n" % (tmp_path / "rec.wav", tmp_path / "more.wav"))
    return str(tmp_path / "wav.scp"), str(tmp_path / "fbank.conf") if stereo else ""


@pytest.mark.parametrize("kind", ["mono", "stereo", "chunks"])
def test_make_segments_device_and_host_legs_write_the_same_directory(tmp_path, kind):
    scp, conf = long_set(tmp_path, stereo=kind == "stereo")
    kw = dict(chunk_frames=100, pass_bytes=70000) if kind == "chunks" else {}
    dirs, counts = {}, {}
    for leg in ("device", "host"):
        out = str(tmp_path / "out")  # (the same name: vad.scp holds the archive's path)
        counts[leg] = ms.make_segments(scp, out, fbank_conf=conf, hip_vad=leg, min_silence=0.05, pad=0.02, **kw)
        dirs[leg] = read_dir(out)
    assert sorted(dirs["device"]) == sorted(ms.NAMES) and dirs["device"] == dirs["host"] and counts["device"] == counts["host"]
    assert counts["device"]["segments"] >= 4 and (kind != "chunks" or counts["device"]["passes"] >= 3)
    if kind != "stereo":
        assert dirs["device"]["segments"].decode().startswith("recA-00000460-00002415 recA 0.460 2.415\nrecA-00002590-00003225 recA 2.590 3.225\n")


def check_lines(seg_lines, cut_lines):
    assert seg_lines == cut_lines and [ln.split()[0] for ln in seg_lines] == [s[0] for s in SEGS]
    assert all(len(ln.split()) > 1 for ln in seg_lines)


@pytest.mark.parametrize("right_ctx", [0, 2])
def test_decode_of_segments_is_decode_of_the_cut_files(tmp_path, monkeypatch, right_ctx):
    scp, seg, cut, _ = segment_set(tmp_path)
    args, state = tiny240() if right_ctx else tiny_case()[:2]
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    for pipelines in (2, 1):
        flags = ["--hip_pipelines", pipelines, "--hip_precision", "fp32"]
        check_lines(run(scp, "--hip_segments", seg, *flags), run(cut, *flags))
    assert run.stats[0]["passes"] >= 1 and not run.stats[2]


def test_decode_of_segments_of_a_stereo_recording_at_another_rate(tmp_path, monkeypatch):
    scp, seg, cut, conf = segment_set(tmp_path, stereo=True)
    args, state = tiny_case()[:2]
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    for pipelines in (2, 1):
        flags = ["--hip_pipelines", pipelines, "--hip_precision", "fp32", "--hip_fbank_conf", conf]
        check_lines(run(scp, "--hip_segments", seg, *flags), run(cut, *flags))


def art_model(tmp_path):
    args, state, _ = ast_tiny_case(ctc_weight=0.3)
    conf = {k: getattr(args, k) for k in ("input_size", "d_model", "n_head", "d_ff", "d_encff", "N_enc", "N_dec", "ctc_weight",
                                          "max_decode_ratio", "T", "ctc_beam", "beam_width", "length_penalty", "decode_type")}
    conf.update(n_features=80, model_type="transformer", beam_width=3, decode_type="ctc_att")
    return write_model(tmp_path, args, state, conf)


def ctm_of(path):
    return [ln.split() for ln in open(path).read().splitlines()]


@pytest.mark.parametrize("task", ["art", "cassnat"])
def test_the_ctm_under_segments_carries_the_recording_and_its_times(tmp_path, monkeypatch, task):
    """Also --task art's result file against the cut files'.  A CTM line of a segment is the cut file's line with the recording's id and
    the segment start (first / rate; multiples of 10 ms here, s-d aside) added, to the printed digit (0.01 s)."""
    scp, seg, cut, _ = segment_set(tmp_path)
    if task == "art":
        ckpt, cfg = art_model(tmp_path)
    else:
        args, state = tiny_case()[:2]
        ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg, task=task, batch_size=2)
    flags = ["--hip_precision", "fp32"]
    a, b = str(tmp_path / "seg.ctm"), str(tmp_path / "cut.ctm")
    check_lines(run(scp, "--hip_segments", seg, "--hip_ctm", a, *flags), run(cut, "--hip_ctm", b, *flags))
    got, want = ctm_of(a), ctm_of(b)
    assert len(got) == len(want) > 0 and {ln[0] for ln in got} == {"recA"} and {ln[0] for ln in want} <= {s[0] for s in SEGS}
    starts = {utt: segments.sample_range(start, end, 16000, SAMPLES)[0] / 16000 for utt, start, end in SEGS}
    for g, w in zip(got, want):
        assert g[1:2] + g[3:] == w[1:2] + w[3:]
        # (the sum is rounded once, the cut file's start was rounded on its own: they agree to the printed digit)
        assert abs(float(g[2]) - starts[w[0]] - float(w[2])) <= 0.0101, (g, w)
        # an aligned unit starts on the 40 ms grid, and a segment start on the 10 ms grid then adds without rounding: the same digits.
        # (A unit that could not be aligned - confidence 0.000, its start a fraction of the frames - can sit on a decimal tie, where
        # the one rounding of the sum and the rounding of the cut file's start may part by the last digit.)
        if w[5] != "0.000" and round(float(w[2]) * 100) % 4 == 0 and w[0] != "s-d":
            assert g[2] == "%.2f" % (starts[w[0]] + float(w[2])), (g, w)
    # without --hip_segments the result lines do not depend on --hip_ctm, and a second CTM of the cut files repeats the first.  (Both
    # runs are this tree's: that the writer's bytes without offsets are what they were is pinned by the hand-written lines of
    # tests/test_segments_host.py::test_the_ctm_writer_with_offsets.)
    assert run(cut, *flags) == run(cut, "--hip_ctm", str(tmp_path / "c.ctm"), *flags) and ctm_of(str(tmp_path / "c.ctm")) == want


@pytest.mark.parametrize("stereo", [False, True])
def test_make_fbank_of_segments_writes_the_archives_of_the_cut_files(tmp_path, stereo):
    scp, seg, cut, conf = segment_set(tmp_path, stereo=stereo)
    dirs = {}
    for name, kw in (("seg", dict(data_path=scp, segments=seg)), ("cut", dict(data_path=cut))):
        out = str(tmp_path / "out")
        c = mf.make_fbank(out_dir=out, fbank_conf=conf, batch_size=3, **kw)
        dirs[name] = read_dir(out)
        assert c["utterances"] == len(SEGS)
    assert dirs["seg"] == dirs["cut"] and dirs["seg"]["utt2num_frames"].decode().split()[0::2] == [s[0] for s in SEGS]


def test_the_chain_make_segments_then_decode(tmp_path, monkeypatch):
    scp, _ = long_set(tmp_path)
    out = str(tmp_path / "vad")
    assert ms.main(["--data_path", scp, "--out_dir", out, "--min_silence", "0.05", "--pad", "0.02", "--max_segment", "1.5"]) == 0
    ids = [ln.split()[0] for ln in open(os.path.join(out, "segments"))]
    assert len(ids) >= 6 and all(i.startswith(("recA-", "recB-")) for i in ids)
    args, state = tiny_case()[:2]
    ckpt, cfg = write_model(tmp_path, args, state, nat_conf(args))
    run = Runs(tmp_path, monkeypatch, ckpt, cfg)
    lines = run(scp, "--hip_segments", os.path.join(out, "segments"), "--hip_precision", "fp32")
    assert [ln.split()[0] for ln in lines] == ids
