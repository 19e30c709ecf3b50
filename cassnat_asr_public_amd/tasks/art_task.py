"""Decode half of the reference's ArtTask (src/tasks/art_task.py:23-66, 233-277): the autoregressive transformer
(BASELINE config 4) behind ``decode_asr.py --task art``.

Same constructor / decode surface and result-file lines ("<utt> tok tok ...").  All three decode types of the reference
(art_task.py:252-259): ``ctc_att`` (joint CTC/attention beam search, src/models/transformer.py:122-241), ``ctc_only`` (CTC prefix
beam search on the encoder, utils.beam_decode.ctc_beam_decode) and ``ctc_correct`` (the decoder as a correction model over the CTC
greedy hypothesis, transformer.py:243-342).  ``ctc_att`` with ``--lm_weight > 0`` fuses the TransformerLM of ``--lm_config`` /
``--rnnlm`` (art_task.py:67-90, transformer.py:186-209) on the device, or - with ``--rank_model n-gram`` and an ARPA text in
``--rnnlm`` - a word n-gram model (models.ngram.NgramLM); LM fusion in ``ctc_only`` / ``ctc_correct`` raises.
A decode step keeps a handful of CUs busy, so a test set goes through
``args.hip_pipelines`` (default 4) engine handles (own workspace + KV cache, ONE shared device copy of the weights) on their
own HIP streams and host threads - batches pulled from the loader by the workers, result lines written in input order.
With torch.distributed initialised (one process per GPU) the utterances are dealt over the ranks by length exactly as
``CassNATTask`` does, rank 0 reads the checkpoint and broadcasts the packed weights over RCCL, and rank 0 writes the one
input-ordered result file - the reference fans out with split_scp.pl and one process + checkpoint read per GPU
(egs/librispeech/run_art.sh:115-135).
"""
import os
import threading
import time

import numpy as np
import torch
import torch.distributed as dist

from .. import dist as cdist
from ..data.segments import rough_frames, utterance_order
from ..data.vocab import Vocab
from ..models import make_conformer, make_transformer
from ..utils import ctm, util
from ..utils.beam_decode import ctc_beam_decode
from .base_task import BaseTask
from .cassnat_task import _is_arpa, hyp_to_words

_DEFAULTS = dict(use_gpu=True, decode_type="ctc_att", use_cmvn=False, dataset_type="SpeechDataset", beam_width=10, ctc_beam=15,
                 ctc_pruning=0, ctc_lp=0, ctc_lm_weight=0, ctc_weight=0.3, max_decode_ratio=0, T=1.0, length_penalty=None, lm_weight=0, left_ctx=0, right_ctx=0,
                 skip_frame=1, padding_idx=0, model_type="transformer", dropout=0.0, rank=0)


class ArtTask(BaseTask):
    def __init__(self, mode, args):
        for k, v in _DEFAULTS.items():
            if not hasattr(args, k):
                setattr(args, k, v)
        super(ArtTask, self).__init__(args)
        if mode != "test":
            raise NotImplementedError("training is out of scope of the accelerated path")
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        self.vocab = Vocab(args.vocab_file, args.rank)
        args.vocab_size = self.vocab.n_words
        args.rank = 0
        for k in ("ctc_alpha", "interctc_alpha", "interctc_layer", "label_smooth"):
            setattr(args, k, 0)
        self.set_model(args)
        self.set_test_dataloader(args, indices=self._shard(args))
        if self.rank == 0:
            self.load_test_model(args.resume_model)
        local = int(os.environ.get("LOCAL_RANK", "0")) if self.world > 1 else 0
        self.model_stats(local, False, False)
        self.lm_model = None

    def _shard(self, args):
        """Indices of this rank's utterances (None = all): the length-sorted snake deal of CassNATTask."""
        if self.world == 1:
            return None
        if getattr(args, "hip_segments", ""):  # (the utterances are the segments: their durations order the list)
            return cdist.shard_indices(np.array(rough_frames(args)), self.world, self.rank)
        n = sum(1 for _ in open(args.test_paths[0]["scp_path"]))
        lengths = np.zeros(n)
        u2n = args.test_paths[0].get("utt2num_frames")
        if u2n:
            lengths = np.array([int(line.split()[1]) for line in open(u2n)])
        return cdist.shard_indices(lengths, self.world, self.rank)

    def set_model(self, args):
        assert args.input_size == (args.left_ctx + args.right_ctx + 1) // args.skip_frame * args.n_features
        if args.model_type == "transformer":
            self.model = make_transformer(args.input_size, args)
        elif args.model_type == "conformer":  # src/tasks/art_task.py:32-35
            self.model = make_conformer(args.input_size, args)
        else:
            raise NotImplementedError("model_type '%s' (the accelerated AST path knows transformer, conformer)" % args.model_type)

    def load_lm_model(self, args):
        """src/tasks/art_task.py:67-90: models.lm.make_model from ``--lm_config`` with the vocabulary's size, weights from the
        ``"state_dict"`` key of ``--rnnlm`` (names with or without the "module." prefix).  The LM runs in the AST's precision.
        Only ``ctc_att`` fuses it (transformer.py:186-209); the CTC prefix beam search's in-loop LM (ctc_lm_weight) is not on the
        accelerated path."""
        self.lm_model = None
        if getattr(args, "ctc_lm_weight", 0) > 0 and getattr(args, "decode_type", "ctc_att") == "ctc_only":
            raise NotImplementedError("CTC beam search with in-loop LM fusion (ctc_lm_weight > 0) is outside the accelerated path")
        if not getattr(args, "lm_weight", 0) > 0:
            return
        if getattr(args, "decode_type", "ctc_att") != "ctc_att":
            raise NotImplementedError("LM fusion with decode_type '%s' is outside the accelerated path (ctc_att fuses the LM)"
                                      % args.decode_type)
        if getattr(args, "rank_model", "lm") == "n-gram":
            # an ARPA text: the package's own word n-gram model, fused in the step loop on the device (every rank reads the file
            # itself); binary kenlm files stay out
            if not _is_arpa(args.rnnlm):
                raise NotImplementedError("rank_model 'n-gram' needs an ARPA text in --rnnlm (a binary kenlm file is not read)")
            from ..models.ngram import NgramLM

            print("Loading n-gram language model from {}".format(args.rnnlm))
            self.lm_model = NgramLM.load(args.rnnlm, self.vocab)
            if torch.cuda.is_available():  # (the tables go up once, before the decode workers start)
                self.lm_model.cuda(getattr(self.model, "_device", None))
            return
        import yaml
        from types import SimpleNamespace

        from ..models.lm import make_model as make_lm_model

        with open(args.lm_config) as f:
            lm_args = SimpleNamespace(**yaml.safe_load(f))
        lm_args.vocab_size = self.vocab.n_words
        lm_args.hip_precision = getattr(args, "hip_precision", "bf16")
        lm_model = make_lm_model(lm_args)
        print("Loading language model from {}".format(args.rnnlm))
        state = torch.load(args.rnnlm, map_location="cpu")["state_dict"]
        with torch.no_grad():
            for name, param in lm_model.named_parameters():
                param.copy_(state[name] if name in state else state["module." + name])
        lm_model.cuda(getattr(self.model, "_device", None))
        self.lm_model = lm_model

    def _lm_engines(self, n, args):
        """One LM handle per pipeline (own step cache), all on the LM's one device copy of the weights."""
        if self.lm_model is None or not hasattr(self.lm_model, "step_engine"):  # (an NgramLM: the workers share its read-only tables)
            return [None] * n
        slots = int(args.batch_size) * int(args.beam_width)
        lm0 = self.lm_model.step_engine(slots)
        return [lm0] + [self.lm_model.new_engine(slots, share=lm0) for _ in range(n - 1)]

    def _engines(self, n, args):
        """n engine handles on ONE device copy of the weights; with several ranks that copy is rank 0's, broadcast once."""
        first = next(iter(self.test_loader))[1] if len(self.test_loader) else None
        frames = max(getattr(args, "hip_max_frames", 4096), first.shape[1] if first is not None else 16)
        eng0 = self.model.build_engine(args.batch_size, frames, with_weights=(self.rank == 0))
        if self.world > 1:
            cdist.broadcast_weights(eng0, src=0)
        return [eng0] + [self.model.new_engine(args.batch_size, frames, share=eng0) for _ in range(n - 1)]

    def decode(self, args):
        # src/tasks/art_task.py:252-259: ctc_only = CTC prefix beam search on the encoder, ctc_correct = the decoder as a
        # correction model over the CTC greedy hypothesis, ctc_att = joint CTC / attention beam search
        if args.decode_type not in ("ctc_att", "ctc_only", "ctc_correct"):
            raise NotImplementedError("decode_type '%s' (ArtTask knows ctc_only, ctc_correct, ctc_att)" % args.decode_type)
        bias_att = False
        if getattr(args, "hip_bias", "") or getattr(args, "hip_bias_model", None) is not None:
            bias_att = getattr(args, "hip_bias_search", "ctc") == "att"
            if bias_att and args.decode_type != "ctc_att":
                raise NotImplementedError("--hip_bias_search att biases the attention beam search (ArtTask: decode_type ctc_att); "
                                          "decode_type '%s' runs no such search" % args.decode_type)
            if not bias_att and args.decode_type != "ctc_only":
                raise NotImplementedError("--hip_bias biases the CTC prefix beam search (ArtTask: decode_type ctc_only); decode_type '%s' "
                                          "runs no such search (--hip_bias_search att biases the attention beam search of ctc_att)"
                                          % args.decode_type)
        if int(getattr(args, "hip_ctc_merge", 0) or 0) and args.decode_type != "ctc_only":
            raise NotImplementedError("--hip_ctc_merge merges the candidates of the CTC prefix beam search (ArtTask: decode_type ctc_only); "
                                      "decode_type '%s' runs no such search" % args.decode_type)
        # (--hip_bias_search att: every pipeline's engine attaches the one list; its tables are shared read-only)
        bias = getattr(args, "hip_bias_model", None) if bias_att else None
        self._args = args
        batch_time = util.AverageMeter("Time", ":6.3f")
        progress = util.ProgressMeter(len(self.test_loader), batch_time)
        n = max(1, min(int(getattr(args, "hip_pipelines", 4)), max(1, len(self.test_loader))))
        engines = self._engines(n, args)
        lm_engines = self._lm_engines(n, args)
        it = iter(enumerate(self.test_loader))
        lock = threading.Lock()
        done = {}
        cv = threading.Condition()
        err = []

        def worker(k):
            try:
                torch.cuda.set_device(getattr(self.model, "_device", 0))
                st = torch.cuda.Stream()
                with torch.cuda.stream(st), torch.no_grad():
                    while not err:
                        with lock:
                            try:
                                i, (utt_list, feats, _, feat_sizes, _) = next(it)
                            except StopIteration:
                                break
                        feats, feat_sizes = self.wave_features(feats, feat_sizes)  # (audio input: fbank on this worker's stream)
                        src_mask = (feats[:, :, 0] != args.padding_idx).unsqueeze(1)
                        if args.decode_type == "ctc_only":
                            recog = ctc_beam_decode(self.model, feats, src_mask, feat_sizes, self.vocab, args, self.lm_model, engine=engines[k])
                        elif args.decode_type == "ctc_correct":
                            recog = self.model.fast_decode_with_ctc(feats, src_mask, self.vocab, args, self.lm_model, engine=engines[k])
                        else:
                            recog = self.model.beam_decode(feats, src_mask, self.vocab, args, self.lm_model, engine=engines[k],
                                                           lm_engine=lm_engines[k], bias=bias)
                        lines = [utt + " " + " ".join(hyp_to_words(seqs[0]["hyp"], self.vocab, args.padding_idx))
                                 for utt, seqs in zip(utt_list, recog)]
                        if getattr(args, "hip_ctm", ""):  # (on this worker's engine and stream, a second encoder pass: utils.ctm)
                            times = ctm.align_batch(self.model, feats, feat_sizes, args, [seqs[0]["hyp"] for seqs in recog], self.vocab,
                                                    engine=engines[k])
                            lines = list(zip(lines, times))
                        with cv:
                            done[i] = lines
                            cv.notify_all()
            except BaseException as e:
                err.append(e)
                with cv:
                    cv.notify_all()

        threads = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(n)]
        end = time.time()
        for t in threads:
            t.start()
        i = -1
        results, times = {}, {}
        for i in range(len(self.test_loader)):
            with cv:
                while i not in done and not err:
                    cv.wait(0.05)
                if err:
                    raise err[0]
                lines = done.pop(i)
            for line in lines:
                if isinstance(line, tuple):  # (--hip_ctm: the line and the utterance's time record)
                    line, rec = line
                    times[line.split(" ", 1)[0]] = rec
                results[line.split(" ", 1)[0]] = line
            batch_time.update(time.time() - end)
            end = time.time()
            if i % args.print_freq == 0 and self.rank == 0:
                progress.print(i)
        for t in threads:
            t.join()
        for e in engines[1:] + [e for e in lm_engines[1:] if e is not None]:
            e.close()
        if i >= 0 and self.rank == 0:
            progress.print(i)
        if self.world > 1:
            gathered = [None] * self.world
            dist.all_gather_object(gathered, results)
            results = {k: v for part in gathered for k, v in part.items()}
            if getattr(args, "hip_ctm", ""):
                gathered = [None] * self.world
                dist.all_gather_object(gathered, times)
                times = {k: v for part in gathered for k, v in part.items()}
        if self.rank == 0:
            order = utterance_order(args)
            with open(args.result_file, "w") as out_file:
                for utt in order:
                    print(results[utt], flush=True, file=out_file)
            if getattr(args, "hip_ctm", ""):
                missed = ctm.write(args.hip_ctm, order, times, ctm.seconds_per_frame(args), ctm.unit_of(args, self.vocab), offsets=self.test_loader.dataset.segment_offsets)
                print("CTM: %d of %d utterances could not be aligned (their units share the frames evenly, confidence 0)" % (missed, len(order)))
            if getattr(args, "hip_score", ""):  # (a post-pass over the words just printed: utils.score)
                from ..utils import score

                score.score_run(args, self.vocab, order, {utt: results[utt].split()[1:] for utt in order})
        return 0
