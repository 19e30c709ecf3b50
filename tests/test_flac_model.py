"""The FLAC model of the tests (tests/flac_model.py): its writer and its reader against each other on every construct the device
decoder is tested with (tests/flac_cases.py), the CRCs against known values, and its reader's refusals.  No GPU."""
import hashlib

import numpy as np
import pytest

import flac_cases as fc
import flac_model as fm


def test_crcs_and_coded_numbers():
    assert fm.crc8(b"123456789") == 0xF4 and fm.crc16(b"123456789") == 0xFEE8  # CRC-8 (0x07) and CRC-16/UMTS (0x8005, MSB first)
    assert fm.coded_number(0) == b"\x00" and fm.coded_number(127) == b"\x7f" and fm.coded_number(128) == b"\xc2\x80"
    assert fm.coded_number(0x7FF) == b"\xdf\xbf" and fm.coded_number(0x800) == b"\xe0\xa0\x80"
    assert len(fm.coded_number((1 << 36) - 1)) == 7 and fm.coded_number((1 << 36) - 1)[0] == 0xFE
    for v in (0, 127, 128, 2047, 2048, 65535, 65536, (1 << 21) - 1, 1 << 21, (1 << 26), (1 << 31), (1 << 36) - 1):
        head = fm.frame_header(v, 192, 0, variable=True)
        data = b"fLaC" + fm.metadata_block(0, fm.streaminfo(16000, 1, 16, 0, 192, 192), last=True) + head
        assert head[-1] == fm.crc8(head[:-1]) and len(head) == 5 + len(fm.coded_number(v))
        del data


@pytest.mark.parametrize("k", range(6))
def test_round_trip_of_every_construct(k):
    u = fc.utterances()[k]
    pcm, info, offsets = fm.read_stream(u["data"])
    np.testing.assert_array_equal(pcm, u["pcm"])
    assert offsets == u["offsets"] and info["channels"] == u["channels"] and info["total"] == len(pcm) and info["bits"] == 16
    assert info["md5"] == hashlib.md5(u["pcm"].tobytes()).digest()
    assert info["min_bs"] == min(u["sizes"]) and info["max_bs"] == max(u["sizes"])


def test_the_cases_hold_what_they_promise():
    by = {u["name"]: u for u in fc.utterances()}
    assert by["sizes"]["sizes"] == [16, 16, 17, 17, 4097, 192, 576, 4096, 4608, 1] and by["types"]["sizes"][-1] == 15
    assert by["stereo"]["pcm"][64:128].tolist() == [[32767, -32768]] * 64 and by["stereo"]["sizes"][-1] == 15
    assert (by["stereo"]["pcm"][128:192].sum(1) % 2 == 1).any()
    assert sorted(set(u["channels"] for u in by.values())) == [1, 2, 3, 8]
    # frames start at each of the four byte alignments of the staged utterance
    assert set(o % 4 for u in by.values() for o in u["offsets"]) == {0, 1, 2, 3}
    runs = fc.unary_run_residuals()
    assert len(runs) == 56 and sorted(set(2 * r if r >= 0 else -2 * r - 1 for r in runs)) == [31, 32, 33, 63, 64, 65, 100]


def test_metadata_blocks_and_unknown_total():
    frames = fm.simple_frames(fc.walk(1000, 2, seed=3), 192, assignment=10)
    seek = b"\xff\xf8\xc9\x18\x00\xc2" * 9  # (sync patterns inside a SEEKTABLE's bytes)
    data, first, offsets, pcm = fm.write_stream(frames, blocks=[(4, b"\x04\0\0\0test\0\0\0\0"), (3, seek), (1, bytes(37))], total=0)
    info, at, blocks = fm.read_metadata(data)
    assert at == first and [k for k, _ in blocks] == [0, 4, 3, 1] and info["total"] == 0
    back, _, offs = fm.read_stream(data)
    np.testing.assert_array_equal(back, pcm)
    assert offs == offsets


def test_the_reader_verifies_crcs_and_md5():
    data, first, offsets, _ = fm.write_stream(fm.simple_frames(fc.walk(500, 1, seed=4), 192))
    for at, what in ((first + 4, "CRC-8"), (first + offsets[1] - 1, "CRC-16"), (4 + 4 + 20, "MD5")):
        bad = bytearray(data)
        bad[at] ^= 0x10
        with pytest.raises(AssertionError, match=what):
            fm.read_stream(bytes(bad))


def test_the_vectorised_writer_round_trips():
    rng = np.random.default_rng(5)
    x = np.clip(np.cumsum(rng.integers(-200, 201, 9001)), -32768, 32767)
    for order, bs in ((2, 4096), (1, 1000), (0, 576)):
        data, first = fm.encode_fast(x, bs=bs, order=order)
        pcm, info, offsets = fm.read_stream(data)
        np.testing.assert_array_equal(pcm[:, 0], x)
        assert info["total"] == 9001 and len(offsets) == -(-9001 // bs) and len(data) < 2 * 9001
