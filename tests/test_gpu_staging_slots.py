"""The packed reader's slot buffers across forms, widths and sizes: ONE staging slot of the decode pipelines takes float32 rows,
compressed payloads and sound samples in turn - unspliced and spliced, so the width of the slot's batch changes 80 <-> 240 -, then
a pass larger than the engines' area and one of more utterances than the slot's per-utterance arrays hold (both must grow), and the
first pass again.  Every pass is held to the definition of its form: ``PackedBatch.padded()`` bit for bit (rows, compressed),
``Fbank.packed`` of every file alone bit for bit (waves)."""
import numpy as np
import pytest
import torch

from test_gpu_compressed_reader import random_payload
from test_gpu_wave_resample import mixed_files, noise
from cassnat_asr_public_amd.data.fbank import Fbank
from cassnat_asr_public_amd.pipeline import DecodePipelines, PackedBatch

pytestmark = pytest.mark.gpu

PAD = -1.5
F0 = 80
LENS = ([5, 23, 40], [31, 7, 12])      # two batches of different longest length; 5, 23, 40, 31 and 7 are no multiples of skip 3
FRAMES = ([3, 17, 33], [25, 8])        # the plain waves' frame counts


def chunks(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


def test_one_slot_takes_every_form_width_and_size():
    from test_gpu_pipeline import build
    from cassnat_asr_public_amd import synth

    args = synth.make_args("tiny")
    args.hip_max_batch, args.hip_max_frames = 4, 90
    model = build(args, synth.make_state(args, seed=0, gain=2.0), "fp32")
    rng = np.random.default_rng(17)
    cmvn = (rng.standard_normal(F0) * 3 + 12, rng.random(F0) + 0.5)
    fbs = {s: Fbank(cmvn_mean=cmvn[0], cmvn_std=cmvn[1], pad_value=PAD, splice=s, channel=1) for s in (None, (0, 2, 1))}
    count = {"compressed_passes": 0, "wave_passes": 0, "resampled_passes": 0, "spliced_passes": 0}

    def mats(lens, seed):
        g = np.random.default_rng(seed)
        return [[(g.standard_normal((n, F0)) * 3 + 11).astype(np.float32) for n in batch] for batch in lens]

    first = mats(LENS, 1)
    payloads = [[random_payload(rng, 1 + (b + i) % 3, n, F0) for i, n in enumerate(batch)] for b, batch in enumerate(LENS)]
    assert {e[0] for batch in payloads for e in batch} == {"CM", "CM2", "CM3"}
    plain = [[(noise(400 + 160 * (n - 1) + 37 * i, 5 + n), 16000, 1) for i, n in enumerate(batch)] for batch in FRAMES]
    files = mixed_files()  # 16 kHz mono, 8 kHz mono, 44.1 kHz stereo, 48 kHz three channels
    other = [files[1:3], files[3:]]

    with DecodePipelines(model, 1, 4, 90, cmvn=cmvn, fbank=fbs[None].o) as pipes:
        pipes._on_gpu, pipes._device = True, torch.cuda.current_device()  # (what the first decode() would set: no worker thread here)

        def stage(pbs):
            feats, ratios = pipes._stage_packed(0, 0, [(pb, pb.ratios(), j) for j, pb in enumerate(pbs)], PAD)
            torch.cuda.synchronize()
            assert tuple(feats.shape) == (sum(pb.shape[0] for pb in pbs), max(pb.shape[1] for pb in pbs), pbs[0].shape[2])
            assert torch.equal(ratios.cpu(), torch.cat([pb.ratios() for pb in pbs]))
            if pbs[0].splice is not None:
                count["spliced_passes"] += 1
            return feats

        def rows_pass(pbs):
            """float32 rows or compressed payloads: every batch's padded() inside a pad-filled (rows, tmax, F) tensor"""
            feats = stage(pbs)
            want = torch.full(tuple(feats.shape), PAD)
            o = 0
            for pb in pbs:
                want[o:o + pb.shape[0], : pb.shape[1]] = pb.padded(PAD, cmvn)
                o += pb.shape[0]
            assert torch.equal(feats.cpu(), want)
            if pbs[0].kinds is not None:
                count["compressed_passes"] += 1
            return feats

        def float_pass(batches, splice=None):
            return rows_pass([PackedBatch(views, splice=splice) for views in batches])

        def wave_pass(batches, splice=None, formats=True):
            fb = fbs[splice]
            pbs, alone = [], []
            for batch in batches:
                each = [fb.packed([chunk], rates=[rate], channels=[C]) for chunk, rate, C in batch]
                alone += [feats[0] for feats, _ in each]
                # (the front-end's frame counts: a spliced file alone has skip 1 here, so its rows are its frames)
                pbs.append(PackedBatch.from_waves([chunk for chunk, _, _ in batch], [a.shape[0] for a in alone[-len(batch):]], F0, splice=splice,
                                                  formats=[(rate, C) for _, rate, C in batch] if formats else None, channel=1 if formats else -1))
            feats = stage(pbs)
            for b, a in enumerate(alone):
                assert torch.equal(feats[b, : a.shape[0]], a), b
                assert (feats[b, a.shape[0]:] == PAD).all()
            count["wave_passes"] += 1
            count["resampled_passes"] += bool(formats)

        one = float_pass(first).clone()                                                             # 1
        assert one.shape[2] == F0
        assert float_pass(first, (0, 2, 1)).shape[2] == 3 * F0                                      # 2: 80 -> 240 in the same slot
        float_pass(first, (1, 1, 3))                                                                # 3
        rows_pass([PackedBatch.from_payloads(batch) for batch in payloads])                         # 4
        rows_pass([PackedBatch.from_payloads(batch, splice=(1, 1, 3)) for batch in payloads])       # 5
        wave_pass(plain, formats=False)                                                             # 6
        wave_pass(plain, (0, 2, 1), formats=False)                                                  # 7
        wave_pass(other)                                                                            # 8
        again = float_pass(first)                                                                   # 9
        assert torch.equal(again, one)
        assert float_pass(mats(LENS, 2)).data_ptr() == again.data_ptr()  # (steady state: an equal-sized pass allocates nothing)
        total = pipes.max_batch * pipes.frames_cap + 1                                              # 10: the data buffers grow
        big = [chunks(total // 2, 45), chunks(total - total // 2, 44)]
        assert sum(map(sum, big)) == total and max(big[0]) != max(big[1])
        float_pass(mats(big, 3))
        many = pipes.max_utts + 1                                                                   # 11: the meta arrays grow
        float_pass(mats([[1] * 40, [1] * (many - 40)], 4))  # (one-row utterances: here the two batches' longest length is the same)
        assert torch.equal(float_pass(first), one)                                                  # 12
        assert pipes.stats["passes"] == 0
        assert {k: pipes.stats[k] for k in count} == count == {"compressed_passes": 2, "wave_passes": 3, "resampled_passes": 1, "spliced_passes": 4}
