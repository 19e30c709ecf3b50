"""Decode FLAC files on the device and compare with the MD5 signature in their STREAMINFO.

    python tools/check_flac_files.py FILE...

For a user who has real FLAC files: every file is indexed on the host (cn_host_flac_index), its frames are decoded by the device
kernels (cn_op_flac_decode) and the MD5 of the interleaved little-endian PCM is compared with the signature the encoder stored.  One
line per file: `OK`, `MISMATCH`, `NO SIGNATURE` (an all-zero MD5: the encoder stored none) or `REFUSED` with the reason; the exit
status is 0 when no file mismatched or was refused.  This is the only check of the decoder against streams this project did not
write itself - its tests decode what their own model of the format (tests/flac_model.py) wrote.
"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decode_file(path, utt=None):
    """-> (interleaved '<i2' PCM (samples, channels) decoded on the device, ``flac_io.Info``)."""
    import torch

    from cassnat_asr_public_amd import hip
    from cassnat_asr_public_amd.data import flac_io
    from cassnat_asr_public_amd.data.fbank import flac_status_error, plan_flac

    info = flac_io.read_info(path, utt)
    if info.bits != 16:
        raise ValueError("%s: %d-bit samples, only 16-bit FLAC streams are read" % (path, info.bits))
    view = flac_io.audio_view(path, info)
    index = flac_io.frame_index(path, info, utt, view)
    plan = plan_flac([index], [0], [info.channels])
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    pcm = torch.zeros(max(16, plan["pcm_bytes"]), dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    hip.flac_decode(dev(np.array(view), torch.uint8), view.shape[0], dev(plan["table"], torch.int32), plan["table"].shape[0], dev(plan["utt"], torch.int32), 1,
                    plan["max_channels"], plan["frame_words"], pcm, plan["pcm_bytes"], status)
    err = flac_status_error(int(status.item()), plan, [utt or os.path.basename(path)])
    if err is not None:
        raise err
    return pcm[:plan["pcm_bytes"]].cpu().numpy().view("<i2").reshape(index.samples, info.channels), info


def check(paths, out=sys.stdout):
    """One line per file -> the number of files that mismatched or were refused."""
    bad = 0
    for path in paths:
        try:
            pcm, info = decode_file(path)
        except (ValueError, OSError) as e:
            print("%s: REFUSED %s" % (path, e), file=out)
            bad += 1
            continue
        got = hashlib.md5(pcm.tobytes()).digest()
        verdict = "NO SIGNATURE" if info.md5 == bytes(16) else ("OK" if got == info.md5 else "MISMATCH")
        bad += verdict == "MISMATCH"
        print("%s: %s  %d samples x %d channels at %d Hz, md5 %s%s" % (path, verdict, pcm.shape[0], pcm.shape[1], info.rate, got.hex(),
                                                                       "" if verdict != "MISMATCH" else " (STREAMINFO: %s)" % info.md5.hex()), file=out)
    return bad


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    sys.exit(1 if check(sys.argv[1:]) else 0)
