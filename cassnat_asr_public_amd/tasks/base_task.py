"""Inference half of the reference's BaseTask (src/tasks/base_task.py:9-149): checkpoint loading by parameter
name, parameter statistics, test dataloader.  Training-side methods are out of scope."""
import torch

from ..data.speech_loader import SpeechDataLoader, SpeechDataset


class BaseTask(object):
    def __init__(self, args):
        self.use_cuda = getattr(args, "use_gpu", True)

    def set_model(self, args):
        raise NotImplementedError

    def load_test_model(self, resume_model):
        """{'model_state': state_dict} with optional 'module.' prefixes (DDP checkpoints), copied by name."""
        if not resume_model:
            return
        print("Loading model from {}".format(resume_model))
        state = torch.load(resume_model, map_location="cpu")["model_state"]
        with torch.no_grad():
            for name, param in self.model.named_parameters():
                param.copy_(state[name] if name in state else state["module." + name])

    def model_stats(self, rank, use_slurm, distributed):
        if distributed:
            raise NotImplementedError("DDP training is out of scope")
        if rank == 0:
            n = sum(p.numel() for p in self.model.parameters())
            print("Number of parameters: {}, updated params: {}".format(n, n))
            self.model_params = self.updated_params = n
        local_rank = rank % max(torch.cuda.device_count(), 1) if use_slurm else rank
        if self.use_cuda:
            torch.cuda.set_device(local_rank)
            self.model = self.model.cuda(local_rank)

    def set_test_dataloader(self, args, indices=None):
        args.use_specaug, args.specaug_conf = False, None
        if getattr(args, "dataset_type", "SpeechDataset") != "SpeechDataset":
            raise NotImplementedError("only the fbank SpeechDataset feeds the accelerated path")
        testset = SpeechDataset(self.vocab, args.test_paths, args)
        if getattr(args, "use_cmvn", False):
            testset._load_cmvn(args.global_cmvn)
        if testset.is_wave:  # audio input: the front-end (and the splice behind it) must produce what the model reads
            left, right, skip = testset.splice() or (0, 0, 1)
            blocks = left + right + 1
            want = int(getattr(args, "n_features", getattr(args, "input_size", testset.num_mel)))
            size = int(getattr(args, "input_size", want))
            # the reference's own agreement (src/tasks/*_task.py set_model: input_size == (left + right + 1) // skip * n_features) and
            # the width the engine is really handed, (left + right + 1) x mel bins; without frame skipping the two together say
            # n_features == mel bins
            if size != blocks // skip * want or size != blocks * testset.num_mel:
                raise ValueError("audio input: the fbank front-end computes %d mel bins, the model reads n_features / input_size = %d / %d"
                                 " (left_ctx / right_ctx / skip_frame = %d / %d / %d: input_size must be %d x n_features and %d x mel bins)"
                                 % (testset.num_mel, want, size, left, right, skip, blocks // skip, blocks))
        self.test_loader = SpeechDataLoader(testset, args.batch_size, args.padding_idx,
                                            num_workers=args.load_data_workers, shuffle=False, indices=indices)
        self._pad_value, self._fbank = float(args.padding_idx), None
        print("Finish Loading test files. Number batches: {}".format(len(self.test_loader)))

    def wave_features(self, feats, feat_sizes):
        """A wave set's batch (``WaveBatch``: int16 samples) -> (feats (B, T, num_mel) cuda, length ratios) on the caller's current
        stream, the global CMVN applied when the dataset has statistics and the frames spliced / skipped when the set asks for it
        (``Fbank.packed``); any other batch passes through."""
        from ..data.speech_loader import WaveBatch

        if not isinstance(feats, WaveBatch):
            return feats, feat_sizes
        fb = getattr(self, "_fbank", None)
        if fb is None:
            from ..data.fbank import Fbank

            ds = self.test_loader.dataset
            o = ds.fbank_opts
            fb = Fbank(cmvn_mean=ds.mean if ds.use_cmvn else None, cmvn_std=ds.std if ds.use_cmvn else None,
                       pad_value=float(getattr(self, "_pad_value", 0.0)), splice=ds.splice(), **ds.wave_admit,
                       **{name: getattr(o, name) for name, _ in o._fields_ if name != "reserved"})
            self._fbank = fb
        if feats.formats is None:
            return fb.packed(feats.views, utts=feats.utts)
        return fb.packed(feats.views, utts=feats.utts, rates=[r for r, _ in feats.formats], channels=[c for _, c in feats.formats],
                         flac=feats.index)
