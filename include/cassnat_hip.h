/* libcassnat_hip.so - C ABI of the MI355X-native CASS-NAT inference hot path.
 *
 * The reference (balaji1312/cassnat_asr_public) is pure Python/PyTorch and has no FFI of its own; the
 * boundary this library sits behind is the Python call
 *     CassNAT.beam_decode(src, x_mask, src_size, vocab, args, ...)      src/models/cassnat.py:420-637
 * made once per batch by CassNATTask.decode                             src/tasks/cassnat_task.py:326-343
 * on a model built by make_model(input_size, args)                      src/models/cassnat.py:21-89
 * whose parameters are loaded by name from {'model_state': ...}         src/tasks/base_task.py:45-54.
 * The Python shim (cassnat_asr_public_amd/models/cassnat.py) binds these entry points with ctypes.
 *
 * Conventions: every function returns 0 on success, a negative code on failure (cn_last_error() gives the
 * text); nothing throws across the ABI.  Pointers named *_dev are device (HBM) pointers owned by the
 * caller; the library owns weights and workspace.  Calls are ordered on the given hipStream_t (passed as
 * void*, NULL = default stream).  One cn_model per device; a handle is not thread-safe.
 */
#ifndef CASSNAT_HIP_H
#define CASSNAT_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cn_model cn_model;

enum { CN_PRECISION_F32 = 0, CN_PRECISION_BF16 = 1, CN_PRECISION_FP8 = 2, CN_PRECISION_BF16X3 = 3, CN_PRECISION_F16 = 4 };
/* CN_PRECISION_F16: the bf16 engine's kernels with IEEE half-precision MFMA operands (11 significant bits instead of 8, same matrix
 * pipe and rate; range +-65504).  It lives in a second build of the same sources, libcassnat_hip_f16.so (-DCN_OP16_F16), which
 * exports this same interface and accepts no other precision; libcassnat_hip.so refuses CN_PRECISION_F16.  cn_operand16() names
 * a library's 16-bit operand ("bf16" / "fp16"). */
enum { CN_DTYPE_F32 = 0, CN_DTYPE_I32 = 1, CN_DTYPE_U8 = 2, CN_DTYPE_F64 = 3 };

/* Model hyper-parameters: the subset of the flat `args` bag that make_model reads for the transformer
 * NAST model (src/models/cassnat.py:41-66). */
typedef struct cn_config {
    int32_t input_size; /* feature dim after splicing (80) */
    int32_t d_model, n_head, d_encff, d_decff;
    int32_t n_enc, n_extra, n_self_dec, n_mix_dec;
    int32_t vocab_size;
    int32_t precision;  /* CN_PRECISION_F32: exact-f32 MFMA (parity gate); CN_PRECISION_BF16: throughput; CN_PRECISION_FP8:
                           the bf16 engine with the encoder layers' products on the e4m3fn MFMA (BASELINE config 5);
                           CN_PRECISION_BF16X3: split-bf16 - every value kept as a bf16 hi + bf16 lo pair (~17 significant
                           bits), every product three bf16 MFMAs (hi.hi + hi.lo + lo.hi, fp32 accumulation): meets the same
                           parity gate as F32 at several times its MFMA rate */
    int32_t max_batch;  /* workspace is sized for max_batch x max_frames */
    int32_t max_frames;
    int32_t device; /* HIP device ordinal */
    int32_t ast;    /* 1: autoregressive (AST) model: n_mix_dec = N_dec decoder layers + tgt_embed (src/models/transformer.py);
                       2: TransformerLM (src/models/lm.py): n_enc layers of width d_encff + text_embed + out_generator.
                       ast = 1 with conf_enc = 1 is the reference's conformer AST model (src/models/conformer.py, pos_type
                       "relative"): the conformer encoder below (enc_max_rel, enc_kernel, d_encff; relative positions, no absolute
                       PE on the source side) under transformer decoder layers whose feed-forward (width d_decff) is Swish with
                       residual scale 1; the target side keeps the absolute sinusoid table.  ast = 1 with conf_dec = 1 and ast = 2
                       with either conformer flag are refused by cn_model_create (the reference defines no such model). */
    /* conformer variants (src/models/cassnat.py:29-57, pos_type "relative"): macaron Swish FFNs, relative-position self
     * attention, convolution module.  conf_enc / conf_dec = args.use_conv_enc / use_conv_dec. */
    int32_t conf_enc, conf_dec;
    int32_t enc_max_rel, dec_max_rel; /* args.enc_max_relative_len / dec_max_relative_len (<= 31) */
    int32_t enc_kernel, dec_kernel;   /* args.enc_kernel_size / dec_kernel_size (odd, >= 1: cn_model_create refuses others) */
    int32_t d_ff;                     /* args.d_ff: width of the conformer extractor's FFN */
    int32_t esa_group;                /* ESA: sampled alignments per utterance one cn_esa_sample pass may take (0/1: one);
                                         sizes the decoder-side workspace (max_batch x esa_group query sets) */
    /* CN_PRECISION_FP8 only: which encoder-side products take e4m3 operands (every e4m3 product adds ~5 % of relative
     * noise to its output; the throughput each one buys differs - DESIGN.md 5d has the measured table).  Bits:
     * CN_FP8_CONV2 the second convolution (conv1 then writes its image in e4m3), CN_FP8_LINEAR linear_out (needs CONV2:
     * conv2 hands its rows on in e4m3), CN_FP8_FFN the two feed-forward products of the encoder layers
     * n >= fp8_ffn_first_layer.  0 = all three, every layer. */
    int32_t fp8_scope;
    int32_t fp8_ffn_first_layer;
} cn_config;
#define CN_FP8_CONV2 1
#define CN_FP8_LINEAR 2
#define CN_FP8_FFN 4

/* Decode-time switches read by beam_decode from `args` (src/models/cassnat.py:435-636). */
typedef struct cn_decode_opts {
    int32_t padding_idx; /* also the CTC blank id */
    int32_t sos;
    int32_t left_trigger, right_trigger;
    int32_t src_trigger;
    int32_t use_unimask;
    int32_t beam_width; /* 1: greedy finish on device; 2..16: per-position top-k kept for the host beam */
    int32_t capture;    /* debug: keep an fp32 copy of every stage tensor for cn_fetch */
    int32_t sub_batch;  /* > 0: the call carries B / sub_batch coalesced batches of that many utterances; the greedy finish limits
                           every hypothesis by the row count of its own batch (src/models/cassnat.py:580-637 reads
                           min(ylen + 1, U of the batch) rows), so each batch's hypotheses are what a call of its own gives.
                           Transformer blocks only (a conformer's GroupNorm sees the padded rows) */
    int32_t no_trigger; /* args.use_trigger == False (src/models/cassnat.py:469-473): the extractor attends over every valid frame
                           (trigger_mask = src_mask) and the row counts are best_path_align's own (no EOS row).  0 = use_trigger */
    int32_t reserved[6]; /* reserved[0] != 0: keep the decoder's full log-probability rows of the pass at any beam_width (what
                            cn_nat_lm_finish reads; beam_width 1 otherwise keeps the arg-max alone).
                            reserved[1] != 0: padded decoder rows.  A greedy pass of a 16-bit engine with the row-chain decoder
                            (d_model 256, transformer blocks; no capture, no use_unimask, use_trigger, no kept rows) otherwise
                            PACKS its decoder side: utterance b owns only the rows its hypothesis reads - min(ylen[b] + 1, row
                            count of its own batch) - one utterance behind the other, instead of U rows each.  Hypotheses,
                            lengths and scores are the same bit for bit either way; the switch is there to compare the two
                            layouts in one library.
                            reserved[2] != 0: the encoder's Q|K|V come from the row-chain launches.  A pass of a 16-bit engine
                            with the row-chain encoder and 128 < T' <= 256 (4 heads, no capture) otherwise projects them inside
                            the self-attention kernel from the LayerNorm rows the chain launches then end with; the results are
                            the same bit for bit, the switch compares the two forms in one library.  The others must be 0 */
} cn_decode_opts;

const char* cn_last_error(void);
const char* cn_version(void);
const char* cn_operand16(void);

/* replaces models.cassnat.make_model (src/models/cassnat.py:21) */
int cn_model_create(const cn_config* cfg, cn_model** out);
/* A further handle on the SAME device copy of the packed weights as the finalized `donor` (reference counted: the last
 * handle to go frees them): own workspace sized by cfg->max_batch / max_frames / esa_group, ready to decode (no load /
 * finalize).  The model hyper-parameters, device and precision must be the donor's.  What the decode pipelines of one GPU
 * use (one engine per pipeline, one 118 MB blob per GPU - and one RCCL broadcast per rank), and what a handle rebuilt for
 * a larger workspace uses.  No reference counterpart: nn.Module parameters are shared by reference in Python. */
int cn_model_create_shared(const cn_config* cfg, cn_model* donor, cn_model** out);
void cn_model_destroy(cn_model* m);

/* replaces the per-parameter copy of BaseTask.load_test_model (src/tasks/base_task.py:50-54): called once per
 * state-dict entry with its reference name ("encoder.layers.0.self_attn.linears.0.weight", ...). fp32 host data. */
int cn_model_load_weights(cn_model* m, const char* name, const float* host_data, const int64_t* shape, int32_t ndim);
/* sinusoid table shared by src_embed.pos_enc.pe and CassNAT.pe (src/models/cassnat.py:91-99): rows x d_model fp32 */
int cn_model_load_pe(cn_model* m, const float* host_table, int32_t rows);
/* repack into MFMA-friendly layouts / model precision and upload; must follow the last load */
int cn_model_finalize(cn_model* m);
/* rank-0 -> all ranks weight hand-off for the multi-GPU path: the packed device blob that RCCL broadcasts */
int cn_model_weight_blob(cn_model* m, void** dev_ptr, int64_t* bytes);

/* replaces CassNAT.beam_decode for the greedy NAST configuration (use_trigger, sample_num <= 1, no LM).
 *   feats_dev      (B,T,F) fp32 contiguous, padded frames exactly == padding_idx in feature 0
 *   size_ratio_dev (B) fp32 length ratios (SuperviseLoader.collate_fn, src/data/speech_loader.py:354)
 *   hyp_out_dev    (B,hyp_stride) int32: [sos, tok...]; hyp_len_dev (B); score_dev (B) float64
 * All stages through the greedy pack run on `stream`; the call synchronises the stream once (the token
 * count U is data dependent).  Workspace: every buffer is checked against the call before anything is launched. */
int cn_decode_nast(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                   const cn_decode_opts* opts, int32_t* hyp_out_dev, int32_t hyp_stride, int32_t* hyp_len_dev,
                   double* score_dev, void* stream);

/* One engine pass over SEVERAL reference batches, each with its own frame count (the reference collates every batch to its own
 * longest utterance, src/data/speech_loader.py:327-356, and decodes batch after batch, src/tasks/cassnat_task.py:317-356):
 * feats_dev holds the batches one after the other, every utterance padded with padding_idx frames to the call's T = the largest
 * sub_frames; batch k has sub_rows_host[k] utterances of sub_frames_host[k] frames (size_ratio relative to THAT count, as
 * collate_fn computes it).  Every utterance's hypothesis and score are exactly those of a cn_decode_nast call on its own batch:
 * its frames past sub_frames are treated as the convolutions' zero padding, src_size = (ratio * T'_own).long()
 * (src/models/cassnat.py:436), the alignment's shift and the forced EOS frame (:355-365, 378-389) use T'_own, keys past T'_own do
 * not exist for the softmax (a row without any allowed key attends uniformly over T'_own keys, attention.py:19-21), and the
 * greedy finish is limited by the row count of the own batch.  n_sub == 0: a plain call (sub_rows / sub_frames unused).
 * Transformer blocks, beam_width 1, no capture.  At most 64 batches per pass.
 * The workspace is an AREA: a pass fits when every buffer holds it (B x T' rows etc. against max_batch x max_frames), so a pass of
 * short utterances may carry more of them than max_batch (up to 16 x max_batch); the error names the buffer that is too small.
 * u_hint > 0: the decoder side is launched on min(u_hint, T' + 1) rows WITHOUT waiting for the data-dependent row count (the
 * reference's `.item()` sync, src/models/cassnat.py:387): nothing in the call blocks the host.  Results equal the exact call's
 * whenever u_hint >= the true count; *ticket_out names the page-locked word that receives the true count - once the stream has
 * drained, cn_decode_ticket(ticket) returns it beside the rows used, and on rows_used < ymax the caller decodes the pass again
 * (u_hint 0 = exact: the call synchronises the stream once, as cn_decode_nast).  A ticket is the call's sequence number on this
 * handle; its counts live in one of FOUR words, so it stays valid until four further decode calls (cn_decode_nast included) have
 * been started on the handle - after that cn_decode_ticket fails ("expired") instead of returning another pass's counts. */
int cn_decode_nast_merged(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                          const cn_decode_opts* opts, int32_t n_sub, const int32_t* sub_rows_host, const int32_t* sub_frames_host,
                          int32_t u_hint, int32_t* hyp_out_dev, int32_t hyp_stride, int32_t* hyp_len_dev, double* score_dev,
                          void* stream, int32_t* ticket_out);
int cn_decode_ticket(cn_model* m, int32_t ticket, int32_t* ymax_host, int32_t* rows_used_host);

/* CN_PRECISION_F16 engines (libcassnat_hip_f16.so): half-precision operands have a range (+-65504).  What drives magnitudes from
 * outside is the scale of the features - everything behind linear_out is LayerNorm-ed in fp32 first -, so every pass compares them
 * with the largest |feature| for which neither subsampling convolution's output can leave half of that range (from the
 * convolutions' weight row sums; a word of the weight blob) and raises a sticky flag.  *fault = 1: a pass since the last call saw
 * such features - its results are not to be used (decode on a bf16 / bf16x3 engine, or normalise the features).  Valid once the
 * passes' stream work is done; clears the flag.  *feature_limit (may be null): that largest |feature|, 0 if unknown.
 * CN_PRECISION_BF16X3 engines use the same guard: their second convolution runs a mixed arithmetic whose e4m3 cross-term operands
 * hold conv1 outputs up to 448 (csrc/conv2.hip MIX); features beyond (448 - |b1|max) / (largest row sum of |w1|) would let them
 * saturate and the engine fall below its tolerance.  Engines of every other precision: *fault = 0. */
int cn_take_range_fault(cn_model* m, int32_t* fault, float* feature_limit);

/* stage-level entry: src_embed + encoder + ctc_generator + alignment only (src/models/cassnat.py:431-468) */
int cn_encode_align(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                    const cn_decode_opts* opts, int32_t* ymax_host, void* stream);

/* ---- autoregressive (AST) model, BASELINE config 4: device half of Transformer.beam_decode (src/models/transformer.py:122-241).
 * The host keeps the beam bookkeeping (as the reference does in Python); per step it passes, for every live hypothesis (row),
 * its last token, utterance index, ancestor table (slot that wrote each earlier position of its prefix) and the key mask of
 * its prefix (token != padding_idx), and receives the top-K of log_softmax(att logits / T).  Keys/values of earlier positions
 * come from a per-layer cache - the decoder is NOT re-run on the whole prefix as the reference does. */
int cn_ast_begin(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts,
                 int32_t want_ctc, int32_t max_len, int32_t max_slots, int32_t ctc_beam, void* stream);
int cn_ast_step(cn_model* m, int32_t n_live, int32_t pos, const int32_t* tok_dev, const int32_t* utt_dev,
                const int32_t* anc_dev, const uint8_t* keyok_dev, int32_t table_stride, float temperature, int32_t K,
                int32_t* topk_idx_dev, float* topk_val_dev, void* stream);
/* CTCPrefixScore.__call__ (src/utils/ctc_prefix.py:50-106) for K candidate labels of every live hypothesis; the new states
 * of all n_live*K candidates are kept on the device (row h*K+c of the buffer of this step's parity) for the next step. */
int cn_ast_ctc_score(cn_model* m, int32_t n_live, int32_t out_len, const int32_t* utt_dev, const int32_t* last_tok_dev,
                     const int32_t* cand_dev, int32_t K, const int32_t* prev_ref_dev, int32_t parity, int32_t eos,
                     float* score_dev, void* stream);

/* LM shallow fusion (src/models/transformer.py:186-209; the LM of src/tasks/art_task.py:67-90): `lm` (a finalized TransformerLM
 * handle, cfg.ast = 2, same vocabulary, device and library; its own precision) runs one incremental step beside every decoder
 * step of `ast` (cfg.ast = 1): the newest position of every slot, keys / values of earlier positions from the LM's own cache
 * [layer][pos][slot][d] (allocated by cn_ast_begin, sized like the decoder's; freed with the LM handle) through the decoder's
 * ancestor and key-mask tables - the reference's lm_model(ys, tgt_mask)[:, -1] with tgt_mask = (ys != padding_idx) &
 * subsequent_mask.  NULL detaches.  The LM handle must stay alive while attached; its workspace (max_batch x max_frames) must
 * hold the beam's slots, its position table max_len.  One LM handle per AST handle (the cache is per handle). */
int cn_ast_attach_lm(cn_model* ast, cn_model* lm);
/* cn_ast_step with the attached LM fused, lm_weight > 0 (after cn_ast_begin):
 * use_ctc == 0 (transformer.py:190-192, 214): topk_idx / topk_val = top-K over V of
 *   log_softmax(att / T) + fl32(lm_weight * log_softmax(lm)) (float32, one rounding per operation; ties: lower index first);
 * use_ctc != 0 (transformer.py:199-209): topk_idx / topk_val = top-K of log_softmax(att / T) as cn_ast_step, and
 *   lm_val_dev [n_live][K] = log_softmax(lm) at those candidates (the caller adds fl32(lm_weight * lm) after the CTC terms). */
int cn_ast_step_lm(cn_model* m, int32_t n_live, int32_t pos, const int32_t* tok_dev, const int32_t* utt_dev,
                   const int32_t* anc_dev, const uint8_t* keyok_dev, int32_t table_stride, float temperature, int32_t K,
                   float lm_weight, int32_t use_ctc, int32_t* topk_idx_dev, float* topk_val_dev, float* lm_val_dev, void* stream);
/* kernel-test entry of the LM step alone: cn_lm_step_begin sizes the LM's step cache; cn_lm_step runs position pos of n rows
 * (tables as cn_ast_step) and writes log_softmax(out_generator(h)) [n][V] fp32 to logp_dev. */
int cn_lm_step_begin(cn_model* lm, int32_t max_len, int32_t max_slots);
int cn_lm_step(cn_model* lm, int32_t n, int32_t pos, const int32_t* tok_dev, const int32_t* anc_dev, const uint8_t* keyok_dev,
               int32_t table_stride, float* logp_dev, void* stream);
/* The LM step with a position per row (cn_ctc_beam_lm's): row h holds tok_dev[h] at position pos_dev[h] <= max_pos and reads
 * pos_dev[h] + 1 keys, key j from cache row rowid_dev[h][j] (any row below max_len * max_slots of cn_lm_step_begin, all keys
 * allowed); a row with stay_dev[h] == 0 writes its K / V to cache row rowid_dev[h][pos_dev[h]], one with stay_dev[h] != 0 writes
 * nothing and its output row is unspecified.  logp_dev [n][V] as cn_lm_step. */
int cn_lm_step_rows(cn_model* lm, int32_t n, int32_t max_pos, const int32_t* tok_dev, const int32_t* pos_dev, const int32_t* stay_dev,
                    const int32_t* rowid_dev, int32_t table_stride, float* logp_dev, void* stream);

/* The whole joint CTC / attention beam search of Transformer.beam_decode (src/models/transformer.py:122-241) on the device,
 * with LM shallow fusion when lm_weight > 0 (an LM attached with cn_ast_attach_lm; an error without one): no host round trip
 * inside the step loop (the host polls a live-hypothesis counter every 8 steps).  1 <= beam_width <= ctc_beam <= 32.
 * hyp_out_dev [B][beam_width][max_len] int32 (sos first, padded with padding_idx), hyp_len_dev [B][beam_width],
 * score_dev [B][beam_width] double; beams best first, same ordering rules as the reference (stable ties). */
typedef struct cn_ast_opts {
    float ctc_weight;            /* > 0: joint scoring with the CTC prefix scorer over ctc_beam candidates */
    float temperature;           /* args.T */
    int32_t ctc_beam;
    int32_t beam_width;
    int32_t max_step;            /* int(max_decode_ratio * T') or T' */
    int32_t eos;
    int32_t use_length_penalty;  /* 0: args.length_penalty is None */
    float one_minus_ctc_weight;  /* float32(1 - ctc_weight) as the reference computes it (in double, then cast) */
    double length_penalty;
    float lm_weight;             /* > 0: LM shallow fusion (args.lm_weight); 0 = no LM.  Takes the place of reserved[0] */
    int32_t reserved[3];
} cn_ast_opts;
int cn_decode_ast(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts,
                  const cn_ast_opts* ast_opts, int32_t* hyp_out_dev, int32_t max_len, int32_t* hyp_len_dev, double* score_dev,
                  void* stream);

/* ---- CASS-NAT + LM: the finish loop of CassNAT.beam_decode with args.lm_weight > 0 (src/models/cassnat.py:574-637) on the device.
 * cn_nat_attach_lm: `lm` (a finalized TransformerLM handle, cfg.ast = 2, same vocabulary, device and library; its own precision,
 * loaded as src/tasks/cassnat_task.py:85-127 loads it) is the lm_model of the finish loop of `nat` (cfg.ast = 0).  NULL detaches.
 * The LM handle must stay alive while attached; its workspace must hold B * beam_width slots, its position table max_len.
 * cn_nat_lm_finish runs the loop (:580-636) after a cn_decode_nast / cn_decode_nast_forced / cn_esa_sample pass of one alignment
 * per utterance that kept its log-probability rows (opts->reserved[0] != 0, or beam_width > 1; a plain pass: not
 * cn_decode_nast_merged with sub-batches or u_hint, not opts->sub_batch > 0 - those are refused): for i < ymax every live hypothesis
 * of an utterance with i <= ylen[b] takes row att_out[b][i] + fl32(lm_weight * lm_model(ys, (ys != padding_idx) & subsequent_mask)
 * [:, -1]) (float32, one rounding per operation), its beam_width best continuations (ties: lower index), and the utterance keeps
 * the beam_width best of them by score + (len(hyp) - 1) * length_penalty (double; the score alone when use_length_penalty == 0;
 * ties in list order).  The LM runs one incremental step per i on every slot b * beam_width + j (keys / values of earlier
 * positions from its cache); nothing returns to the host inside the loop.  ymax: the reference's ymax (<= the rows of the pass;
 * ESA: the largest ylen of the selected samples).  zero_past_len != 0: rows i >= ylen[b] read as all-zero (ESA, :536).
 * 1 <= beam_width <= 16; beam_width 1 takes the arg-max of the fused row (not the greedy path of cn_decode_nast).
 * hyp_out_dev [B][beam_width][max_len] int32 (sos first, padded with padding_idx; max_len >= ymax + 1), hyp_len_dev [B][beam_width],
 * score_dev [B][beam_width] double; beams best first. */
int cn_nat_attach_lm(cn_model* nat, cn_model* lm);
int cn_nat_lm_finish(cn_model* m, const cn_decode_opts* opts, int32_t ymax, int32_t beam_width, float lm_weight,
                     int32_t use_length_penalty, double length_penalty, int32_t zero_past_len, int32_t* hyp_out_dev, int32_t max_len,
                     int32_t* hyp_len_dev, double* score_dev, void* stream);

/* ---- ESA: error-based sampling of alignments + TransformerLM ranking (src/models/cassnat.py:370-376, 441-445, 499-561) --
 * cn_esa_begin: encoder + CTC generator once; the two best labels of every frame are kept.
 * cn_esa_sample: n_samples (<= cfg.esa_group) sampled alignments per utterance in one pass: in alignment g, frame t of
 * utterance b takes the second-best label iff select[g][b][t] != 0 and the best label's probability < threshold (all-zero
 * draws - or select_dev == NULL with n_samples == 1 - give the best path); then alignment -> extractor -> decoder ->
 * generator over B * n_samples query sets that share the B utterances' encoder outputs: tok_out / val_out
 * [n_samples][B][out_stride] = argmax token and its log-probability per decoder row, ylen_out [n_samples][B] (EOS row
 * included), *ymax_host = rows of this pass.  force_U: 0 = decode on this pass's own row count; > 0 = on that many rows
 * (conformer blocks: GroupNorm sees an utterance's padded rows, so every group must use the row count of ALL samples, as the
 * reference's single batch does); -1 = count only (outputs may be NULL).  The caller owns the random draws (the reference takes them from
 * torch.randint) and loops over groups of samples.  opts->beam_width must be 1. */
int cn_esa_begin(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts, void* stream);
int cn_esa_sample(cn_model* m, const uint8_t* select_dev, int32_t n_samples, float threshold, const float* size_ratio_dev,
                  const cn_decode_opts* opts, int32_t* tok_out_dev, float* val_out_dev, int32_t out_stride,
                  int32_t* ylen_out_dev, int32_t* ymax_host, int32_t force_U, void* stream);
/* TransformerLM (src/models/lm.py; model created with cfg.ast = 2: n_enc layers of width d_encff, parameters
 * text_embed.0.lut / encoder.* / out_generator.proj): score[b][u] = log p(tgt[b][u] | tok[b][0..u]) with key j allowed
 * iff j <= u and j < len[b].  tok / tgt / score are [B][ld] with ld >= U. */
int cn_lm_score(cn_model* m, const int32_t* tok_dev, const int32_t* tgt_dev, const int32_t* len_dev, int32_t B, int32_t U,
                int32_t ld, float* score_dev, void* stream);

/* ---- decode_type ctc_only / ctc_att (src/tasks/cassnat_task.py:335-341) ------------------------------------------------
 * cn_ctc_beam replaces utils.beam_decode.ctc_beam_decode (src/utils/beam_decode.py:8-93) without a language model: encoder,
 * CTC generator, the `pruning` best labels per frame, then the prefix beam search over the frames (frames past src_size and
 * frames with blank probability > 0.95 skipped, candidates not merged by prefix, stable sort by score_ctc + length_penalty *
 * len(hyp), float64 scores) on the device.  hyp_out_dev [B][beam][hyp_cap] labels (no sos; hyp_cap >= T' + 1), hyp_len_dev /
 * score_dev (score_ctc) / p_blk_dev / p_nblk_dev [B][beam], nbeam_dev [B] hypotheses kept, best first. */
int cn_ctc_beam(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                const cn_decode_opts* opts, int32_t beam, int32_t pruning, double length_penalty, int32_t* hyp_out_dev,
                int32_t hyp_cap, int32_t* hyp_len_dev, double* score_dev, double* p_blk_dev, double* p_nblk_dev, int32_t* nbeam_dev,
                void* stream);
/* The same search with the TransformerLM in the frame loop (ctc_beam_decode(..., lm_model) with args.ctc_lm_weight): m a CASS-NAT
 * or autoregressive handle with a CTC head, lm a finalized cfg.ast = 2 handle of the same library, device and vocabulary (an
 * argument: independent of cn_nat_attach_lm / cn_ast_attach_lm).  One loop iteration per processed frame - LM step with a position
 * per row on all B * beam slots, the LM rows of the beam, the frame step -, queued by the host without a read-back; the host reads
 * the iteration count (the largest number of processed frames of an utterance; *iterations_host when not NULL) once before the
 * loop.  score_lm is the reference's running sum: the j-th non-blank candidate of a hypothesis carries the parent's score_lm plus
 * double(lm_prob[c]) * lm_weight over the non-blank pruned labels up to its own, in list order; the sort key is (score_ctc +
 * score_lm) + length_penalty * len(hyp).  The LM's step cache takes iterations x B x beam rows per layer; the LM handle needs
 * max_batch x (max_frames / 4 + 1) >= B x beam and a position table of iterations + 1 rows.  Outputs as cn_ctc_beam, plus
 * score_lm_dev [B][beam].  With opts->capture the log-posteriors the search ran on are kept (cn_fetch "ctc_out"). */
int cn_ctc_beam_lm(cn_model* m, cn_model* lm, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                   const cn_decode_opts* opts, int32_t beam, int32_t pruning, double length_penalty, double lm_weight,
                   int32_t* hyp_out_dev, int32_t hyp_cap, int32_t* hyp_len_dev, double* score_dev, double* score_lm_dev,
                   double* p_blk_dev, double* p_nblk_dev, int32_t* nbeam_dev, int32_t* iterations_host, void* stream);
/* CassNAT.beam_decode for decode_type 'ctc_att' with sample_num 1 (src/models/cassnat.py:446-448): the trigger mask comes from
 * the forced (Viterbi) alignment of labels_dev [B][ld] / label_len_dev [B] (beam_path_align -> viterbi_align, :391-414,
 * 272-353) instead of the greedy path; max_label_len = the largest label_len (the width of the reference's label tensor).
 * Outputs as cn_decode_nast. */
int cn_decode_nast_forced(cn_model* m, const float* feats_dev, const float* size_ratio_dev, int32_t B, int32_t T, int32_t F,
                          const cn_decode_opts* opts, const int32_t* labels_dev, const int32_t* label_len_dev, int32_t ld,
                          int32_t max_label_len, int32_t* hyp_out_dev, int32_t hyp_stride, int32_t* hyp_len_dev, double* score_dev,
                          void* stream);
/* ESA ranking with rank_model 'at_baseline' (src/models/cassnat.py:514-520, Transformer.forward_decoder): the autoregressive
 * model (cfg.ast = 1, cfg.esa_group >= n_per_utt) scores token rows teacher-forced: its encoder on the B utterances, then the
 * decoder on N = B * n_per_utt rows (row e belongs to utterance e % B) under the causal + length mask:
 * score[e][u] = log softmax(att_generator(dec_h[e][u]))[tgt[e][u]].  tok / tgt / score [N][ld], ld >= U. */
int cn_ast_teacher_score(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts,
                         const int32_t* tok_dev, const int32_t* tgt_dev, const int32_t* len_dev, int32_t n_per_utt, int32_t U,
                         int32_t ld, float* score_dev, void* stream);

/* ArtTask decode_type 'ctc_correct' = Transformer.fast_decode_with_ctc (src/models/transformer.py:243-342, called at
 * src/tasks/art_task.py:254-255): the CTC greedy hypothesis (arg-max path zeroed on masked frames, repeats collapsed, blanks dropped)
 * behind sos is the teacher-forced decoder input under the causal + padding mask; returned are the hypothesis lengths len_out_dev [B]
 * and, for the U = longest + 1 decoder rows (*rows_host), the k best labels and log-probabilities of every row, tok_out_dev /
 * val_out_dev [B][U][k] (buffers of B * (T' + 1) * k entries): what the reference's finish loop (:276-341) consumes on the host. */
int cn_ast_ctc_correct(cn_model* m, const float* feats_dev, int32_t B, int32_t T, int32_t F, const cn_decode_opts* opts, int32_t k,
                       int32_t* tok_out_dev, float* val_out_dev, int32_t* len_out_dev, int32_t* rows_host, void* stream);

/* Copy a named internal / captured tensor to the host (synchronous; test + host-beam use).  Activations are
 * returned as fp32 whatever the model precision.  shape_out has room for 4 dims. */
int cn_fetch(cn_model* m, const char* name, void* host_dst, int64_t max_bytes, int64_t* shape_out, int32_t* ndim_out,
             int32_t* dtype_out);

/* Per-kernel timing with HIP events recorded on the launch stream around each tagged kernel.
 * tags: '|'-separated list ("conv2|self_attention") or NULL for every tag.  cn_profile_end synchronises the device and
 * writes {"tag": {"count": n, "ms": total, "flops": algorithmic flops, "bytes": algorithmic bytes}, ...}. */
int cn_profile_begin(cn_model* m, const char* tags);
int cn_profile_end(cn_model* m, char* json_out, int64_t cap);

/* Row-chain kernel (bf16, d_model 256), one launch for the non-attention half of a layer on 128-row blocks:
 * x += Wo.ctx + bo (skipped when ctx_dev is NULL); x += W2.relu(W1.LN1(x)+b1)+b2 (skipped when dff == 0);
 * when nln_a_host != NULL: out = Wt.LNn(x)+bt (tail_n columns) or out = LNn(x) itself (tail_n == 0), bf16 [M][ldo].
 * Replaces linears[3] + SublayerConnection + PositionwiseFeedForward + LayerNorm + linears[0..2]
 * (src/models/modules/attention.py:44-66, utils.py:23-32, positionff.py:15-16, norm.py:15-18).  Weights are host fp32
 * in nn.Linear layout and are packed on every call: a test entry point, the model keeps its packed copies.
 * x_mode bits (each a field of cn_chain_desc below, which states every layout in one place): 1 = x_dev is read in the kernel's
 * blocked layout, 2 = written in it, 4 = not written back, 8 = the feed-forward
 * activation is Swish (x * sigmoid(x), the conformer's macaron halves) instead of ReLU, 16 = the tail projection out_dev is
 * written as a blocked bf16 matrix of ldo columns (ceil(M / 32) * 32 rows; 32 x 32 tiles of 2 KiB, each [16-column half][lane =
 * 32 * (bit 3 of the column) + row % 32][8 bf16]: what the attention kernel reads as `blocked` Q / K / V).  Blocked x: 32-row
 * blocks of [32 pieces i][64 lanes][4 floats], lane = row % 32 + 32 h holding channels 32 (i / 4) + 8 (i % 4) + 4 h + (0..3);
 * the buffer then holds ceil(M / 32) * 32 rows.  32 = the two feed-forward products take e4m3fn operands (BASELINE config 5,
 * CN_PRECISION_FP8 engines; d_ff % 256 == 0, ReLU only): LN1(x) at x16 and the ReLU output at x8, both saturating at +-448,
 * W1 and W2 each at the largest power-of-two scale that keeps its largest magnitude <= 448; accumulation, bias, residual and
 * everything else of the launch as without the bit.  64 (with tail_n == 0, ldo == 256) = LNn(x) goes to out_dev as the kernel's
 * own B operands: per 32-row block [16 k-steps][lane = row % 32 + 32 h][8 values], value j of (k-step ks, h) being channel
 * 32 (ks / 2) + 16 (ks % 2) + 8 (j / 4) + 4 h + j % 4; ceil(M / 32) * 32 rows - what cn_op_attention_proj (cassnat_hip_attention_proj.h) reads as y_dev. */
int cn_op_chain(float* x_dev, const void* ctx_dev, int32_t ldctx, const float* wo_host, const float* bo_host,
                const float* ln1_a_host, const float* ln1_b_host, const float* w1_host, const float* b1_host,
                const float* w2_host, const float* b2_host, const float* nln_a_host, const float* nln_b_host,
                const float* wt_host, const float* bt_host, void* out_dev, int32_t ldo, int32_t M, int32_t dff,
                int32_t tail_n, float eps, int32_t x_mode, void* stream);
/* cn_op_chain whose row count lives on the device: M sizes the grid (and the buffers), *rows_dev <= M rows exist - workgroups
 * past them leave at once, the guards use the device value (the packed decoder side's launches). */
int cn_op_chain_rows(float* x_dev, const void* ctx_dev, int32_t ldctx, const float* wo_host, const float* bo_host,
                     const float* ln1_a_host, const float* ln1_b_host, const float* w1_host, const float* b1_host,
                     const float* w2_host, const float* b2_host, const float* nln_a_host, const float* nln_b_host,
                     const float* wt_host, const float* bt_host, void* out_dev, int32_t ldo, int32_t M, int32_t dff,
                     int32_t tail_n, float eps, int32_t x_mode, const int32_t* rows_dev, void* stream);
/* Every option of the row-chain kernel (the internal ChainArgs), the one place that states its fields and layouts; cn_op_chain
 * and cn_op_chain_rows are this entry with the x_mode bits spelled out.  One launch, on the library's 16-bit operand type (bf16,
 * or IEEE half in libcassnat_hip_f16):
 *   x += Wo.ctx + bo                      if ctx != NULL
 *   x += W2.act(W1.LN1(x) + b1) + b2      if dff > 0 (act: ReLU, or Swish = v * sigmoid(v) with `swish`)
 *   y = LNn(x)                            if nln_a != NULL; LayerNorm of the reference: unbiased std, eps added to the std
 *   out = Wt.y + bt (tail_n > 0) or out = y (tail_n == 0); ln_out = y as well where it is given.
 * Weights (wo [256][256], w1 [dff][256], w2 [256][dff], wt [tail_n][256], the biases and LayerNorm vectors) are HOST fp32 in
 * nn.Linear layout, packed on every call: a test entry.  dff % 128 == 0 <= 2048, tail_n % 256 == 0 <= 1536.  M rows; with
 * rows_dev (a device word, ReLU forms only) M sizes the grid and the buffers, *rows_dev <= M rows exist and workgroups past them
 * write nothing.  store_x == 0: x is read and not written back.  f8: the two feed-forward products on e4m3fn operands as x_mode
 * bit 32 of cn_op_chain describes (dff % 256 == 0, ReLU only).
 * Layouts (device buffers; a blocked buffer holds ceil(M / 32) * 32 rows, and the rows of the last 32-row block past M may be
 * written with values of no meaning):
 *   x       row-major fp32 [M][256]; x_in_blocked / x_out_blocked: read / written as 32-row blocks of [32 pieces i][64 lanes]
 *           [4 floats], lane = row % 32 + 32 h holding channels 32 (i / 4) + 8 (i % 4) + 4 h + (0..3)
 *   ctx     row-major [M][ldctx] of 16-bit values (the first 256 columns are read); ctx_blocked (ldctx == 256): the attention
 *           kernel's o_blocked output - per 32-row block [16 k-steps][lane = row % 32 + 32 h][8 values], value j of (k-step ks, h)
 *           being channel 16 ks + 8 h + j
 *   out     row-major [M][ldo] of 16-bit values; out_blocked (tail_n > 0, ldo % 32 == 0): a blocked matrix of ldo columns -
 *           32 x 32 tiles of 2 KiB, each [16-column half][lane = 32 * (bit 3 of the column) + row % 32][8 values], what the
 *           attention kernel reads as `blocked` Q / K / V
 *   ln_out  row-major [M][ld_ln] of 16-bit values, written IN ADDITION to a tail (the last encoder layer: enc_h beside the
 *           decoder side's K|V); NULL: none.  ln_blocked (256 columns: ld_ln == 256, or ldo == 256 where `out` takes y): y goes
 *           out - to ln_out, or to `out` of a launch without tail - as the kernel's own B operands: per 32-row block
 *           [16 k-steps][lane = row % 32 + 32 h][8 values], value j of (k-step ks, h) being channel
 *           32 (ks / 2) + 16 (ks % 2) + 8 (j / 4) + 4 h + j % 4 - what cn_op_attention_proj reads as y_dev.
 * cn_chain_desc_size() is sizeof(cn_chain_desc). */
typedef struct cn_chain_desc {
    float* x;
    const void* ctx;
    int32_t ldctx, ctx_blocked;
    const float* wo;
    const float* bo;
    const float* ln1_a;
    const float* ln1_b;
    const float* w1;
    const float* b1;
    const float* w2;
    const float* b2;
    const float* nln_a;
    const float* nln_b;
    const float* wt;
    const float* bt;
    void* out;
    void* ln_out;
    int32_t ldo, ld_ln;
    int32_t M, dff, tail_n;
    float eps;
    int32_t ln_blocked, out_blocked, store_x, x_in_blocked, x_out_blocked, swish, f8;
    const int32_t* rows_dev;
} cn_chain_desc;
int cn_op_chain_desc(const cn_chain_desc* d, void* stream);
int32_t cn_chain_desc_size(void);

/* ---- front-end: waveform -> log-mel filterbank features (+ global CMVN), padded batch out ----------------------
 * What the reference leaves to Kaldi's compute-fbank-feats (egs/librispeech/conf/fbank.conf:1-6: hamming window, 16 kHz,
 * 80 mel bins, no energy; other options at Kaldi's defaults, dither = 0) followed by the (feat - mean) / std of
 * SpeechDataset._load_cmvn (src/data/speech_loader.py:109-115).  wave_dev: [B][max_samples] float32 on the int16 scale
 * (as Kaldi reads a wav); num_samples_dev: [B]; feats_dev: [B][Tmax][num_mel] float32, frame t of utterance b exists for
 * t < 1 + (num_samples[b] - frame_len) / frame_shift (snip_edges), later frames are filled with pad_value (the
 * decoder's padding_idx, so that its mask derivation feats[:,:,0] != padding_idx sees them as padding).
 * cmvn_mean_dev / cmvn_istd_dev: [num_mel] or NULL.  The output is directly cn_decode_nast's feats_dev. */
typedef struct cn_fbank_opts {
    float sample_rate, frame_length_ms, frame_shift_ms, preemph, low_freq, high_freq;
    int32_t num_mel, window_type /* 0 hamming, 1 povey, 2 hanning, 3 rectangular */, remove_dc, use_power, use_log;
    int32_t reserved[5];
} cn_fbank_opts;
void cn_fbank_default_opts(cn_fbank_opts* o);
int32_t cn_fbank_num_frames(const cn_fbank_opts* o, int32_t num_samples);
int cn_fbank(const cn_fbank_opts* o, const float* wave_dev, const int32_t* num_samples_dev, int32_t B, int32_t max_samples,
             const float* cmvn_mean_dev, const float* cmvn_istd_dev, float* feats_dev, int32_t Tmax, float pad_value,
             void* stream);
/* The same front-end behind the packed reader (audio input): staged_dev holds the utterances' little-endian int16 samples exactly as
 * the WAV `data` chunks hold them, utterance r (samples_dev[r] samples) at BYTE offset off_dev[r], a multiple of 16.  Frame t of
 * utterance r exists for t < cn_fbank_num_frames(samples[r]); out_dev[r][t][:] (rows, T, num_mel) is cn_fbank's value for it bit for
 * bit (the two kernels share the frame arithmetic; int16 -> float is exact) and `pad` for later t.  With statistics (float64,
 * [num_mel]) the value stored is float((double(e) - mean) / std): cn_op_unpack_rows' arithmetic, not cn_fbank's float32 form - audio
 * plus global CMVN equals an `FM ` archive of the un-normalised features plus the same CMVN.  Nothing outside [0, staged_bytes) is
 * read.  Refused without a launch: a null pointer, rows / T / num_mel <= 0, a frame of more than 512 samples. */
int cn_op_fbank_packed(const cn_fbank_opts* o, const void* staged_dev, int64_t staged_bytes, const int32_t* off_dev,
                       const int32_t* samples_dev, float* out_dev, int32_t rows, int32_t T, float pad, const double* mean_dev,
                       const double* std_dev, void* stream);
/* cn_op_fbank_packed for float32 samples on the int16 scale (the wave cn_op_wave_resample writes): utterance r (samples_dev[r]
 * samples) at BYTE offset off_dev[r] of wave_dev, a multiple of 16.  The two forms are one kernel, a template on the sample type:
 * for the same float values this one, cn_op_fbank_packed and cn_fbank agree bit for bit.  Nothing outside [0, wave_bytes) is read;
 * the same refusals. */
int cn_op_fbank_packed_f32(const cn_fbank_opts* o, const void* wave_dev, int64_t wave_bytes, const int32_t* off_dev,
                           const int32_t* samples_dev, float* out_dev, int32_t rows, int32_t T, float pad, const double* mean_dev,
                           const double* std_dev, void* stream);

/* ---- front-end: sample-rate conversion and channel pick in front of fbank ---------------------------------------
 * What Kaldi's compute-fbank-feats does with a file whose rate differs from --sample-frequency (--allow-downsample /
 * --allow-upsample: ResampleWaveform) or that holds several channels (--channel).  The arithmetic is LinearResample with
 * num_zeros = 6 and cutoff = 0.99 * 0.5 * min(in_rate, out_rate): with g = gcd(in_rate, out_rate), in_unit = in_rate / g and
 * out_unit = out_rate / g (the number of phases), phase i has the weights w[i][j] = filt(d) * win(d) / in_rate for the input
 * indices j = first[i] .. last, first[i] = ceil((i / out_rate - W) * in_rate), last = floor((i / out_rate + W) * in_rate),
 * d = j / in_rate - i / out_rate, W = num_zeros / (2 cutoff), and output k = u * out_unit + i of a wave x is
 * sum_j w[i][j] x[first[i] + u * in_unit + j] with x = 0 outside the wave.  The tables are built on the host in double and rounded
 * to float32 once; the kernel accumulates in float32 in ascending j (fmaf), so that per output
 * |y - exact| <= (taps + 3) * 2^-24 * sum_j |w_j x_j|.  Equal rates: one weight 1.0, the output is exactly float(x).
 * Host only: cn_resample_num_samples is the number of outputs for in_samples inputs (GetNumOutputSamples with flush = true:
 * ceil(in_samples * out_unit / in_unit); 0 for a non-positive argument).  cn_resample_table gives the table exactly as the device
 * gets it: first_host / taps_host [out_unit], weights_host [max_taps][out_unit] (tap-major; zero behind a phase's taps), `capacity`
 * = the floats weights_host can hold; with the three arrays null only in_unit / out_unit / max_taps are set.  It refuses what
 * cn_op_wave_resample refuses of a rate pair. */
int64_t cn_resample_num_samples(int32_t in_rate, int32_t out_rate, int64_t in_samples);
int cn_resample_table(int32_t in_rate, int32_t out_rate, int32_t* in_unit, int32_t* out_unit, int32_t* max_taps,
                      int32_t* first_host, int32_t* taps_host, float* weights_host, int64_t capacity);
/* The utterances of ONE source rate, in one launch.  staged_dev: the layout cn_op_fbank_packed reads - utterance r's data chunk as
 * its file holds it (interleaved little-endian int16, channels[r] channels of samples[r] samples each) at BYTE offset off_dev[r], a
 * multiple of 16.  Channel channel[r] of it is converted from in_rate to out_rate and written as float32 to wave_dev +
 * out_off_dev[r] (an offset in FLOATS, a multiple of 4): cn_resample_num_samples(samples[r]) values, nothing else - gaps and other
 * utterances' slots are not touched.  The per-utterance arrays have `utts` entries; rows_dev (device, `rows` utterance indices) names
 * the utterances of this call - a pass that mixes rates makes one call per rate - or is NULL: utterances 0 .. rows - 1.  max_out:
 * the longest output count among them (it sizes the grid).  channels_host / channel_host: the same values as channels_dev /
 * channel_dev, on the host, checked before the launch.  Nothing outside [0, staged_bytes) is read: an utterance whose offset and
 * length reach outside is cut to the samples that lie inside.  Refused without a launch: a null pointer, a non-positive rate, utts,
 * rows or max_out, a channel outside [0, channels), more than 65535 rows, a rate pair whose table has more than 65536 weights or
 * of which 256 consecutive outputs need more input samples than the kernel's LDS tile holds (4096).  The tables are kept per
 * (device, in_rate, out_rate). */
int cn_op_wave_resample(int32_t in_rate, int32_t out_rate, const void* staged_dev, int64_t staged_bytes, const int32_t* off_dev,
                        const int32_t* samples_dev, const int32_t* channels_dev, const int32_t* channel_dev,
                        const int32_t* channels_host, const int32_t* channel_host, int32_t utts, const int32_t* rows_dev,
                        int32_t rows, int64_t max_out, float* wave_dev, const int32_t* out_off_dev, void* stream);

/* ---- single-kernel entry points (parity tests drive each hand-written kernel through the ABI) ---------- */
/* all pointers device; `precision` selects the element type of activations/weights: CN_PRECISION_F32, CN_PRECISION_BF16 or
 * CN_PRECISION_BF16X3 (split-bf16 elements: each group of 32 consecutive elements of a row is 128 bytes, 32 bf16 hi halves
 * then 32 bf16 lo halves; rows and row strides are multiples of 32 elements) */
/* fp32 <-> a flat tensor of n elements in the given precision's element type (to_f32 = 0: src fp32 -> dst; 1: back) */
int cn_op_convert(int32_t precision, const void* src, void* dst, int64_t n, int32_t to_f32, void* stream);
int cn_op_gemm(int32_t precision, const void* A, int32_t lda, const void* W, const float* bias, void* C, int32_t ldc,
               int32_t c_is_f32, int32_t M, int32_t N, int32_t K, int32_t relu, const float* resid, int32_t ldr,
               const float* pe, int32_t pe_period, float scale, void* stream);
/* The tiled GEMM (csrc/gemm.hip) through a descriptor that reaches every field of its non-convolution product - what cn_op_gemm
 * cannot express: Swish, resid_scale, e4m3 operands with a 16-bit / fp32 / e4m3 output, the device-side weight scale:
 *     v = (A . W^T) * deq + bias          deq = 1, or acc_scale * (w_inv_scale ? *w_inv_scale : 1) with e4m3 operands (ab_fp8)
 *     RELU: v = max(v, 0);  SWISH: v = v * sigmoid(v);  EMBED: v = v * scale + (pe ? pe[m % pe_period][n] : 0)
 *     RESID: v = resid[m][n] + resid_scale * v;  e4m3 output: v = v * c_scale, saturating at +-448;  C[m][n] = round(v)
 * in that order, `epi` being a sum of CN_GEMM_EPI_* bits.  All operands are device pointers in the kernel's own storage, nothing is
 * packed by the call: A [M][lda] and W [N][K] (K contiguous) in the element type of `precision` (CN_PRECISION_F32 / BF16 / BF16X3 /
 * F16; with ab_fp8: e4m3fn bytes, `precision` CN_PRECISION_BF16 naming the 16-bit output type), bias [N], resid [M][ldr] and pe
 * [pe_period][N] fp32 (resid may alias an fp32 C), C [M][ldc] of c_kind: CN_GEMM_OUT_OWN (the element type; 16-bit with ab_fp8),
 * CN_GEMM_OUT_F32 or CN_GEMM_OUT_E4M3 (ab_fp8 only).  Strides in elements.  resid_scale, scale, acc_scale and c_scale are used as
 * given (a zeroed descriptor has none of them at 1).  Rows >= M and columns >= N (of A: >= K) are neither read nor written.
 * cn_gemm_form is the host-only decision of which kernel such a call takes, without touching the device: elem | out << 4 | tile << 8
 * of the CN_GEMM_ELEM_*, CN_GEMM_OUT_*, CN_GEMM_TILE_* enumerators (CN_GEMM_TILE_NONE: M or N is 0, nothing is launched;
 * CN_GEMM_TILE_LINEAR256: the LDS-DMA linear_out kernel of the front end takes the call), or -1 where cn_op_gemm_desc would refuse.
 * The engine's own products go through the same decision.
 * Refused with a message that starts "cn_op_gemm_desc: " (cn_gemm_form: "cn_gemm_form: "), before anything is launched: a null
 * descriptor, null A, W or C; a precision this library does not own; unknown epilogue bits or output kind, a non-zero reserved
 * word; an e4m3 output without e4m3 operands; e4m3 operands in another precision than CN_PRECISION_BF16; M or N < 0; a K that is
 * not a positive multiple of the slab (32 fp32 / 64 sixteen-bit / 32 split / 128 e4m3); an lda that does not keep rows 16-byte
 * aligned; lda < K, ldc < N; RESID without resid or with ldr < N; split-bf16 strides (lda; ldc of a split output) that are not
 * multiples of 32.  M == 0 or N == 0: returns 0, launches nothing.  cn_gemm_desc_size() is sizeof(cn_gemm_desc). */
enum { CN_GEMM_EPI_RELU = 1, CN_GEMM_EPI_RESID = 2, CN_GEMM_EPI_EMBED = 4, CN_GEMM_EPI_SWISH = 8 };
enum { CN_GEMM_ELEM_F32 = 0, CN_GEMM_ELEM_16 = 1, CN_GEMM_ELEM_SPLIT = 2, CN_GEMM_ELEM_E4M3 = 3 };
enum { CN_GEMM_OUT_OWN = 0, CN_GEMM_OUT_F32 = 1, CN_GEMM_OUT_E4M3 = 2 };
enum { CN_GEMM_TILE_NONE = 0, CN_GEMM_TILE_128 = 1, CN_GEMM_TILE_64 = 2, CN_GEMM_TILE_64_FULLK = 3, CN_GEMM_TILE_LINEAR256 = 4,
       CN_GEMM_TILE_CONV = 5, CN_GEMM_TILE_CONV2_DMA = 6 };
typedef struct cn_gemm_desc {
    int32_t precision, c_kind;
    const void* A;
    const void* W;
    const float* bias;
    void* C;
    const float* resid;
    const float* pe;
    const float* w_inv_scale;
    int32_t lda, ldc, ldr;
    int32_t M, N, K;
    int32_t epi, pe_period;
    float resid_scale, scale;
    int32_t ab_fp8;
    float acc_scale, c_scale;
    int32_t reserved;
} cn_gemm_desc;
int cn_op_gemm_desc(const cn_gemm_desc* d, void* stream);
int32_t cn_gemm_desc_size(void);
int32_t cn_gemm_form(const cn_gemm_desc* d);
int cn_op_conv1(int32_t precision, const float* x, const float* w9c, const float* bias, void* out, int32_t B, int32_t T,
                int32_t F, int32_t C, void* stream);
/* the bf16 engine's form of the same layer (src/models/modules/embedding.py:102-104): conv1 + ReLU written as the bordered bf16
 * image [B][T1+2][F1+2][C] (zero border) that the second convolution's tile kernel reads; computed on the matrix cores from
 * split-bf16 operands (16 significant bits in front of the bf16 rounding).  C == 256, (F-1)/2 + 3 >= 32. */
int cn_op_conv1_bordered(const float* x, const float* w9c, const float* bias, void* out, int32_t B, int32_t T, int32_t F,
                         int32_t C, void* stream);
/* fp8 engine's conv front-end (BASELINE config 5, src/models/modules/embedding.py:102-108 on e4m3fn operands): conv1 + ReLU written as
 * an e4m3fn image at img_scale (a power of two; saturating), conv2 + ReLU from it with w2 (HOST fp32, [C][3][3][C]: k = (kh*3+kw)*C + ci)
 * quantised at the largest power-of-two scale that keeps max|w| <= 448 (returned in *w_scale_out); out bf16 [B*T2*F2][C].  C == 256.
 * img8_out_dev (optional): the image as the second kernel reads it, [B][T1+2][F1+2][C] bytes with its border of zeros. */
int cn_op_conv_frontend_fp8(const float* x_dev, const float* w1_9c_dev, const float* b1_dev, const float* w2_host,
                            const float* b2_dev, void* out_dev, void* img8_out_dev, int32_t B, int32_t T, int32_t F, int32_t C,
                            float img_scale, float out8_scale, float* w_scale_out, void* stream);

/* The split-bf16 engine's conv front-end in its MIX arithmetic (csrc/conv2.hip): a product is half(a) half(b) + l_a q_b + q_a l_b
 * with l = e4m3((v - half(v)) S_l) and q = e4m3(v S_q) at fixed power-of-two scales - one half-precision MFMA plus two e4m3 MFMAs
 * at twice the rate where the split-bf16 form spends three bf16 MFMAs.  x fp32 [B][T][F] (device), w1 [9][C] / b1 / b2 device,
 * w2_host fp32 [C][3][3][C] (k = (kh * 3 + kw) * C + ci); out: split-bf16 rows [B * T2 * F2][C] (device).  C = 256. */
int cn_op_conv_frontend_mix(const float* x, const float* w1_9c, const float* b1, const float* w2_host, const float* b2, void* out,
                            void* img_out /* optional: conv1's planes, 4 bytes per bordered cell */, int32_t B, int32_t T, int32_t F,
                            int32_t C, void* stream);
/* (out8_scale > 0: out_dev receives e4m3fn bytes [B*T2*F2][C] at that scale instead of bf16 - the input of the next entry)
 * linear_out (src/models/modules/embedding.py:118-119) of the fp8 engine: a8_dev [M][K] e4m3fn at a_scale, K = 5120; w_host fp32
 * [256][K] quantised at the largest power-of-two scale in range (*w_scale_out); out fp32 [M][256] =
 * (a . w^T + bias) * out_scale + pe[m % pe_period] (pe_dev may be NULL). */
int cn_op_linear256_fp8(const void* a8_dev, const float* w_host, const float* bias_dev, float* out_dev, int32_t M, int32_t K,
                        float a_scale, float out_scale, const float* pe_dev, int32_t pe_period, float* w_scale_out, void* stream);
int cn_op_conv2(int32_t precision, const void* conv1_out, const void* w_khwc, const float* bias, void* out, int32_t B,
                int32_t T1, int32_t F1, int32_t C, void* stream);
/* Every launch form of the subsampling front end (csrc/conv1.hip, conv2.hip, gemm.hip; src/models/modules/embedding.py:102-119)
 * from one descriptor - what the entries above cannot reach: per-utterance records of a merged pass, halo modes 1 and 2, each
 * conv1 kernel by name, conv2's split-bf16 planes form, linear_out with a padded row stride.  A stage runs where its form is not 0;
 * the stages run in the order conv1, conv2, linear and are independent but for the image.
 *   precision  CN_PRECISION_F32 / BF16 / BF16X3 (libcassnat_hip.so) or F16 (libcassnat_hip_f16.so): the element type of the plain
 *              conv1 form, of the generic conv2 and linear forms and of the 16-bit tile forms' operands
 *   conv1      x [B][T][F] fp32, w9c [9][C] fp32 (tap-major), bias1 [C]: device.  The image `img` (device) is the CALLER's and is
 *              NOT cleared: [B][T1][F1][C] elements (halo 0) or [B][T1+2][F1+2][C] (halo 1: the border zeros are written; halo 2:
 *              they are there already - interior cells only, and the rows past an utterance's own batch).
 *              T1 = (T-1)/2+1, F1 = (F-1)/2+1.  CN_FE_CONV1_PLAIN: the VALU kernel in `precision` (split-bf16: halo 0 only);
 *              PLANES: bordered bf16 hi plane, then the lo plane; MIXPLANES: bordered half-precision hi values (2 bytes per cell),
 *              then the bytes e4m3((v - hi) img_scale), then e4m3(v img_scale2); F8_VALU / F8_MFMA: bordered e4m3 bytes at
 *              img_scale, from the VALU or the matrix-core kernel; BF16_MFMA: the bordered 16-bit image from the matrix-core kernel
 *              (the two matrix-core forms: C == 256, 32 <= F1 + 2 <= 65; they write their border always: halo == 1).
 *              n_sub > 0: sub_rows / sub_frames (HOST, n_sub <= 64 entries, rows summing to B, 1 <= frames <= T) are the batches
 *              of a merged pass; the entry expands them on the device (launch_expand_meta) into B records {frames, tp, sub_lo,
 *              sub_hi}, hands those to conv1 and copies them to meta_out (device, B x 4 int32; may be NULL).
 *   conv2      reads `img` ([B][T1(+2)][F1(+2)][C] as above, from the conv1 stage or filled by the caller), w2 HOST fp32
 *              [C][3][3][C] (k = (kh * 3 + kw) * C + ci) packed per call with the library's own packers, bias2 [C] device ->
 *              c2_out [B * T2 * F2][C].  CN_FE_CONV2_GENERIC: launch_gemm's implicit GEMM as the engine calls it (halo 0: the
 *              plain image in `precision`; halo != 0: the engine's bordered call, which the tile kernel takes); DMA: the tile
 *              kernel on the bordered 16-bit image; X3: on the two bordered planes, split-bf16 rows out; MIX: on the three
 *              planes, split-bf16 rows out; F8: on the bordered e4m3 image at img_scale, 16-bit rows out, or with out8_scale > 0
 *              e4m3 bytes at that scale.  The tile forms need C == 256.
 *   linear     lin_out fp32 [M][256] = (lin_a . lin_w^T + lin_bias) * scale + pe[m % pe_period] (pe may be NULL).  lin_a device
 *              [M][lda] (CN_FE_LINEAR_F8: e4m3 bytes at a_scale, lda == K == 5120), lin_w HOST fp32 [256][K], lin_bias, pe
 *              device.  GENERIC: launch_gemm with the embedding epilogue as the engine calls it; DMA: launch_linear256_dma.
 *   q8_out     (HOST, 8 int32, may be NULL) the E8M0 scale bytes chosen: [0..3] conv2's (F8: {W, image}; MIX: {W_q, A_l, W_l,
 *              A_q}), [4..7] linear's ({W, A}).
 * Refused with a message that starts "cn_op_frontend_desc: ", before anything is packed or launched: a null descriptor; no stage;
 * a form or precision this library does not have; a form whose shape rule fails; a halo the form does not have (0 on an
 * always-bordered form, 2 on a form that writes its border always, any on the plain split-bf16 image); a conv2 form that does not
 * read what the conv1 form writes; a rows list that does not sum to B, has more than 64 entries or frames outside 1 .. T.
 * cn_frontend_desc_size() is sizeof(cn_frontend_desc). */
enum { CN_FE_CONV1_PLAIN = 1, CN_FE_CONV1_PLANES = 2, CN_FE_CONV1_MIXPLANES = 3, CN_FE_CONV1_F8_VALU = 4, CN_FE_CONV1_F8_MFMA = 5,
       CN_FE_CONV1_BF16_MFMA = 6 };
enum { CN_FE_CONV2_GENERIC = 1, CN_FE_CONV2_DMA = 2, CN_FE_CONV2_X3 = 3, CN_FE_CONV2_MIX = 4, CN_FE_CONV2_F8 = 5 };
enum { CN_FE_LINEAR_GENERIC = 1, CN_FE_LINEAR_DMA = 2, CN_FE_LINEAR_F8 = 3 };
typedef struct cn_frontend_desc {
    int32_t precision, conv1_form, conv2_form, linear_form;
    const float* x;
    const float* w9c;
    const float* bias1;
    int32_t B, T, F, C;
    int32_t halo, n_sub;
    float img_scale, img_scale2;
    const int32_t* sub_rows;
    const int32_t* sub_frames;
    void* meta_out;
    void* img;
    const float* w2;
    const float* bias2;
    void* c2_out;
    float out8_scale;
    int32_t lda;
    const void* lin_a;
    const float* lin_w;
    const float* lin_bias;
    float* lin_out;
    int32_t M, K;
    float a_scale, scale;
    const float* pe;
    int32_t pe_period, reserved;
    int32_t* q8_out;
} cn_frontend_desc;
int cn_op_frontend_desc(const cn_frontend_desc* d, void* stream);
int32_t cn_frontend_desc_size(void);
int cn_op_layernorm(int32_t precision, const float* x, const float* a2, const float* b2, void* y, int32_t M, int32_t d,
                    float eps, void* stream);
/* The conformer convolution module's kernels one at a time (csrc/conformer.hip; src/models/modules/conformer_related.py:15-44).
 * "The precision's layout": fp32, the library's 16-bit operand, or split-bf16 rows (per group of 32 columns 32 hi then 32 lo
 * halves; d % 32 == 0).  Each entry refuses, before any launch: null pointers; M, B, L, d or k < 1; M * d (L * d) beyond the
 * kernels' int arithmetic; split-bf16 with d % 32 != 0.
 * cn_op_glu: in [M][2d] -> out [M][d] = in[:, :d] * sigmoid(in[:, d:]), both in the precision's layout. */
int cn_op_glu(int32_t precision, const void* in, void* out, int32_t M, int32_t d, void* stream);
/* Depthwise convolution over time: y[b][t][c] = bias[c] + sum_j w[c][j] x[b][t + j - (k - 1) / 2][c], zero outside [0, L) of the
 * same utterance.  x [B*L][d] in the precision's layout; w [d][k], bias [d], y [B*L][d] fp32.  Any k >= 1 (an even k has the
 * longer side of its window behind t; cn_model_create refuses it for a model).  form 0: the launcher's choice (the tiled kernel for
 * k = 3, 7, 15, 31, the naive one otherwise), 1: the naive kernel. */
int cn_op_dwconv(int32_t precision, const void* x, const float* w, const float* bias, float* y, int32_t B, int32_t L, int32_t d,
                 int32_t k, int32_t form, void* stream);
/* GroupNorm(1, d) over the whole L x d image of each utterance (biased variance), affine per channel, Swish.  x [B*L][d] fp32;
 * stats [B][2] float64, written by the call: (sum, sum of squares) of each utterance; gw, gb [d] fp32; out [B*L][d] in the
 * precision's layout. */
int cn_op_groupnorm_swish(int32_t precision, const float* x, double* stats, const float* gw, const float* gb, void* out, int32_t B,
                          int32_t L, int32_t d, float eps, void* stream);
int cn_op_attention(int32_t precision, const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V,
                    int32_t ldv, void* O, int32_t ldo, int32_t B, int32_t H, int32_t Lq, int32_t Lk,
                    const uint8_t* keymask, const int32_t* klen, const int32_t* intervals, int32_t iv_stride,
                    int32_t causal, float scale, void* stream);
/* Every option of the fused attention kernel (the internal AttnArgs, field for field): Q / K / V / O rows of the precision's
 * elements with head h at columns 64h.. (row-major: ld* >= 64 * H); keymask [entries][Lk]; kv_mod > 0 / kv_index: query set b
 * reads K / V / keymask / kcap of entry b % kv_mod / kv_index[b]; klen [B]; kcap: entry e holds kcap[e * kcap_stride] <= Lk keys,
 * later ones are absent (-inf); q_blocked / kv_blocked / o_blocked (16-bit layouts, no rel_pos): blocked matrices of q_n / kv_n /
 * ldo columns, head 0 at q_col / k_col / v_col; intervals [B][iv_stride][4]; causal; rel_pos [2R+1][ld_pos] fp32 with rel_u /
 * rel_v [64 H] fp32 (relative-position self attention, Lq == Lk, R <= 31).  cn_attn_desc_size() is sizeof(cn_attn_desc). */
typedef struct cn_attn_desc {
    const void* Q;
    const void* K;
    const void* V;
    void* O;
    int32_t ldq, ldk, ldv, ldo;
    int32_t B, H, Lq, Lk;
    const uint8_t* keymask;
    int32_t kv_mod;
    const int32_t* kv_index;
    const int32_t* klen;
    const int32_t* kcap;
    int32_t kcap_stride;
    int32_t q_blocked, kv_blocked;
    int32_t q_col, k_col, v_col, q_n, kv_n;
    int32_t o_blocked;
    const int32_t* intervals;
    int32_t iv_stride;
    int32_t causal;
    float scale;
    const float* rel_pos;
    const float* rel_u;
    const float* rel_v;
    int32_t rel_R, ld_pos;
} cn_attn_desc;
int cn_op_attention_desc(int32_t precision, const cn_attn_desc* a, void* stream);
int32_t cn_attn_desc_size(void);
/* The same kernel on PACKED query rows: entry b owns row_off_dev[b + 1] - row_off_dev[b] <= Lq rows of Q and O from row
 * row_off_dev[b] on (row-major or blocked) instead of Lq rows from b * Lq on; Lq only sizes the grid; `intervals` keeps its
 * [B][iv_stride] layout.  kv_packed != 0 (self attention: Lq == Lk, no keymask / kv_mod / kv_index): K / V entry b likewise
 * holds its own count of keys from row_off_dev[b] on; keys at or past the count are absent and never loaded. */
int cn_op_attention_packed(int32_t precision, const cn_attn_desc* a, const int32_t* row_off_dev, int32_t kv_packed, void* stream);
/* Row plan of a packed decoder side: r[b] = min(ylen[b] + 1, limit, hyp_stride - 1), the rows cn_op_greedy_pack reads, with
 * limit = min(U, *ymax_dev if non-null, largest ylen of b's own batch: utt_meta_dev [B][4] int32 (frames, T', first utterance,
 * one past the last) if non-null, else blocks of `sub` utterances if 0 < sub < B, else the whole call);
 * row_off_dev[0 .. B] = exclusive prefix sum of r (row_off_dev[B]: the total). */
int cn_op_row_plan(const int32_t* ylen_dev, int32_t B, int32_t U, int32_t hyp_stride, int32_t sub, const int32_t* utt_meta_dev,
                   const int32_t* ymax_dev, int32_t* row_off_dev, void* stream);
int cn_op_logsoftmax_argmax(float* logits, int32_t M, int32_t V, int32_t* arg, float* maxlp, int32_t write_logp,
                            void* stream);
/* The plain form of cn_op_ctc_align_desc (include/cassnat_hip_align.h: every form, and the layouts).  Like it, this entry refuses
 * (-1, message set, nothing written) a null pointer, B < 1 or Tp < 1 - the launcher behind it returns 0 for an empty call. */
int cn_op_ctc_align(const int32_t* best, const uint8_t* keymask, const float* size_ratio, int32_t B, int32_t Tp,
                    int32_t blank, int32_t left, int32_t right, int32_t* shift, int32_t* src_size, int32_t* ylen,
                    int32_t* ymax, int32_t* intervals, void* stream);
/* CTC prefix beam search (src/utils/beam_decode.py:8-93, no LM) and forced alignment (src/models/cassnat.py:272-345: the label of
 * the aligned state per frame, before the collapse / shift that cn_op_ctc_align's kernel applies) on given log-posteriors
 * logp [B][Tp][V]; buffers as cn_ctc_beam / cn_decode_nast_forced */
int cn_op_ctc_prefix_beam(const float* logp, const float* size_ratio, int32_t B, int32_t Tp, int32_t V, int32_t beam, int32_t pruning,
                          double length_penalty, int32_t blank, int32_t* hyp, int32_t hyp_cap, int32_t* hyp_len, double* score,
                          double* p_blk, double* p_nblk, int32_t* nbeam, void* stream);
int cn_op_ctc_viterbi(const float* logp, const uint8_t* keymask, const float* size_ratio, const int32_t* labels,
                      const int32_t* label_len, int32_t B, int32_t Tp, int32_t V, int32_t ld, int32_t ymax, int32_t blank,
                      int32_t* out_path, void* stream);
/* cn_op_greedy_pack_rows (include/cassnat_hip_align.h) without row limits.  Refuses (-1, message set) a null pointer, B < 1, U < 1
 * or hyp_stride < 1 - the launcher behind it returns 0 for an empty call. */
int cn_op_greedy_pack(const int32_t* tok, const float* val, const int32_t* ylen, int32_t B, int32_t U, int32_t sos,
                      int32_t hyp_stride, int32_t* hyp, int32_t* hyp_len, double* score, void* stream);
/* fused LN -> W1 -> ReLU -> W2 -> residual (-> next LN) sublayer, bf16 / d_model 256.  x_dev fp32 [M][256] is updated
 * in place; weights are HOST fp32 nn.Linear matrices (w1 [dff][256], w2 [256][dff]) packed and uploaded by the call
 * (test entry: the model packs once at cn_model_finalize).  xn_out_dev (bf16 [M][256]) may be NULL.  nslice > 1: the
 * hidden units are split over nslice workgroups per row tile and a second kernel adds the slices (the form the
 * autoregressive decode step uses for its few rows); d_ff % (128 * nslice) == 0. */
int cn_op_ffn_fused(float* x_dev, const float* ln_a_dev, const float* ln_b_dev, const float* w1_host,
                    const float* b1_dev, const float* w2_host, const float* b2_dev, const float* nln_a_dev,
                    const float* nln_b_dev, void* xn_out_dev, int32_t M, int32_t dff, float eps, int32_t nslice,
                    void* stream);
/* the same sublayer in the split-bf16 precision (CN_PRECISION_BF16X3; fused_x3.hip): three MFMAs per product on hi + lo
 * operands; xn_out_dev is split-bf16 [M][256] (or NULL).  mix != 0: the sublayer's two products in the engine's mixed arithmetic
 * instead (what the engine runs) - half(a) half(b) + l_a q_b + q_a l_b with e4m3 l = (v - half(v)) 2^11 S and q = v S: one
 * half-precision MFMA per 16 k and one K = 64 e4m3 MFMA per 32 k, 2 MFMA units per product */
int cn_op_ffn_x3(float* x_dev, const float* ln_a_dev, const float* ln_b_dev, const float* w1_host, const float* b1_dev,
                 const float* w2_host, const float* b2_dev, const float* nln_a_dev, const float* nln_b_dev, void* xn_out_dev,
                 int32_t M, int32_t dff, float eps, int32_t mix, void* stream);
/* The two sublayers above with a choice of hidden activation: act = CN_ACT_RELU (what cn_op_ffn_fused / cn_op_ffn_x3 run) or
 * CN_ACT_SWISH, h * sigmoid(h) on h = W1 . LN(x) + b1 with residual scale 1 - the decoder feed-forward of the conformer AST model
 * (src/models/conformer.py:30).  cn_op_ffn_x3_act: Swish needs mix == 0 (the engine runs Swish in the plain split form only). */
enum { CN_ACT_RELU = 0, CN_ACT_SWISH = 1 };
int cn_op_ffn_fused_act(float* x_dev, const float* ln_a_dev, const float* ln_b_dev, const float* w1_host,
                        const float* b1_dev, const float* w2_host, const float* b2_dev, const float* nln_a_dev,
                        const float* nln_b_dev, void* xn_out_dev, int32_t M, int32_t dff, float eps, int32_t nslice,
                        int32_t act, void* stream);
int cn_op_ffn_x3_act(float* x_dev, const float* ln_a_dev, const float* ln_b_dev, const float* w1_host, const float* b1_dev,
                     const float* w2_host, const float* b2_dev, const float* nln_a_dev, const float* nln_b_dev, void* xn_out_dev,
                     int32_t M, int32_t dff, float eps, int32_t mix, int32_t act, void* stream);
/* the row-chain form of the split-bf16 engine (fused_x3.hip): attention output projection + residual, feed-forward sublayer, next
 * LayerNorm and (wt_host != null) the next attention's projection of it, in one launch; ctx_dev split-bf16 [M][256] or null;
 * weight matrices on the host, vectors on the device (positionff.py:15-16, attention.py:57-66, norm.py:15-18).  Refused before
 * anything is packed or uploaded: d_ff not a multiple of 128 in [128, 2048]; with wt_host a tail_n that is not a multiple of 128
 * in [128, 1024], no next LayerNorm (the tail projects LN_next(x)), no bt_dev or tail_out_dev; ctx_dev without wo_host / bo_dev */
int cn_op_x3_chain(float* x_dev, const void* ctx_dev, const float* wo_host, const float* bo_dev, const float* ln_a_dev,
                   const float* ln_b_dev, const float* w1_host, const float* b1_dev, const float* w2_host, const float* b2_dev,
                   const float* nln_a_dev, const float* nln_b_dev, void* xn_out_dev, const float* wt_host, const float* bt_dev,
                   void* tail_out_dev, int32_t tail_n, int32_t M, int32_t dff, float eps, int32_t mix /* as cn_op_ffn_x3 */,
                   void* stream);
/* fused generator tail, bf16 / d_model 256: arg[m] = argmax_v, maxlp[m] = max_v of log_softmax(W h[m] + b); h_dev bf16 [M][256],
 * W/b HOST fp32 nn.Linear parameters (packed and uploaded by the call; the model packs once at cn_model_finalize).  This entry
 * and the two below are plain forms of cn_op_genmax_desc (include/cassnat_hip_genmax.h: every form, the refusals - theirs start
 * with their own names - and the gather's contract for a target outside the vocabulary). */
int cn_op_genmax(const void* h_dev, const float* w_host, const float* b_host, int32_t M, int32_t V, int32_t* arg_dev,
                 float* maxlp_dev, void* stream);
/* the same kernel with a target gather (TransformerLM scoring, src/models/cassnat.py:507-520): h_dev bf16 [B * U][256];
 * tgt_lp[b * ld + u] = log_softmax(W h[b * U + u] + b)[tgt[b * ld + u]] */
int cn_op_genmax_gather(const void* h_dev, const float* w_host, const float* b_host, int32_t B, int32_t U, int32_t V,
                        const int32_t* tgt_dev, int32_t ld, float* tgt_lp_dev, void* stream);
/* the generator tail in the split-bf16 precision (CN_PRECISION_BF16X3; three MFMAs per product): h_host fp32 [M][256] (split
 * and uploaded by the call).  tgt_dev == NULL: arg-max (and maxlp when maxlp_dev != NULL); else M = B * U rows and
 * tgt_lp[b * ld + u] = log_softmax(W h[b * U + u] + b)[tgt[b * ld + u]] */
int cn_op_genmax_x3(const float* h_host, const float* w_host, const float* b_host, int32_t M, int32_t V, int32_t* arg_dev,
                    float* maxlp_dev, const int32_t* tgt_dev, int32_t U, int32_t ld, float* tgt_lp_dev, void* stream);
/* d_model-deep projection of the split-bf16 engine (proj_x3.hip; the nn.Linear layers around the attention kernel,
 * src/models/modules/attention.py:57-66): a_host fp32 [M][256], w_host fp32 [N][256] (split into hi + lo halves, packed and
 * uploaded by the call), bias_host [N]; N a multiple of 32, at most 1024.  split_out == 0: c_dev fp32 [M][N] = A . W^T + bias,
 * or resid + resid_scale * (...) when resid_dev (fp32 [M][N], may alias c_dev);  split_out == 1: c_dev receives split-bf16
 * rows (M * N * 4 bytes: per 32 columns 64 bytes of bf16 hi halves, then 64 bytes of lo halves) */
int cn_op_proj_x3(const float* a_host, const float* w_host, const float* bias_host, const float* resid_dev, float resid_scale,
                  void* c_dev, int32_t M, int32_t N, int32_t split_out, void* stream);
/* The same projection through a descriptor that reaches every field of the launch (cn_op_proj_x3 is a caller of it): a_dev is on
 * the DEVICE already, M rows of 256 split-bf16 elements at a row stride of lda elements (4 bytes each: per 32 elements 64 bytes of
 * hi halves, then 64 bytes of lo halves); w_host fp32 [N][256] and bias_host [N] are packed and uploaded by the call; c_dev fp32
 * [M][ldc] (split_out == 0) or split-bf16 rows of ldc elements (split_out == 1); resid_dev fp32 [M][ldr] or null, fp32 output
 * only, may alias c_dev: C = resid + resid_scale * (A . W^T + bias).  Strides in elements.  Rows >= M, columns >= 256 of A and
 * >= N of C and resid are neither read nor written.
 * Refused with a message that starts "cn_op_proj_x3_desc: ", before anything is packed or touches the device: a null descriptor,
 * null a_dev, w_host, bias_host or c_dev; a non-zero reserved word; M < 0; split_out other than 0 / 1; N not a multiple of 32 in
 * [32, 1024]; lda not a multiple of 32; lda < 256; ldc < N; a split output whose ldc is not a multiple of 32; a residual with a
 * split output or with ldr < N; an fp32 output beyond 2 GiB.  The three stride bounds are the launcher's own (launch_proj_x3), so
 * the engine's calls are held to them as well.  M == 0: returns 0, launches nothing.
 * cn_proj_x3_form: what such a call launches, decided on the host alone - *mt = 32-row tiles per workgroup (2 from M = 4096 on),
 * *chunks = column chunks (gridDim.y: the fewest c with N / 32 divisible by 4 c that reach 256 workgroups, else the most); -1 for
 * M < 1 or an N the kernel does not take. */
typedef struct cn_proj_x3_desc {
    const void* a_dev;
    const float* w_host;
    const float* bias_host;
    void* c_dev;
    const float* resid_dev;
    int32_t lda, ldc, ldr;
    int32_t M, N;
    int32_t split_out;
    float resid_scale;
    int32_t reserved;
} cn_proj_x3_desc;
int cn_op_proj_x3_desc(const cn_proj_x3_desc* d, void* stream);
int32_t cn_proj_x3_desc_size(void);
int cn_proj_x3_form(int32_t M, int32_t N, int32_t split_out, int32_t* mt, int32_t* chunks);
/* Which of its nine instantiations the split-bf16 feed-forward kernel (fused_x3.hip) runs for a call of cn_op_ffn_x3_act /
 * cn_op_x3_chain, decided on the host alone: *form = a sum of CN_FFN_X3_PRO (ctx: the output projection in front), CN_FFN_X3_TAIL
 * (tail_n != 0: the next projection behind), CN_FFN_X3_MIX and CN_FFN_X3_SWISH.  -1 with a message where the launch is refused: a
 * tail_n that is not a multiple of 128 in [128, 1024], Swish with mix, ctx or a tail, an unknown act. */
enum { CN_FFN_X3_PRO = 1, CN_FFN_X3_TAIL = 2, CN_FFN_X3_MIX = 4, CN_FFN_X3_SWISH = 8 };
int cn_ffn_x3_form(int32_t has_ctx, int32_t tail_n, int32_t mix, int32_t act, int32_t* form);
int cn_op_topk(const float* logp, int32_t M, int32_t V, int32_t k, int32_t* idx, float* val, void* stream);
/* e4m3fn product (BASELINE config 5): A bf16 [M][lda] on the device is quantised at a_scale (saturating at 448 / a_scale),
 * W = HOST fp32 [N][K] at the largest power-of-two scale that fits (returned in *w_scale_out), as cn_model_finalize does for
 * the encoder layers of a CN_PRECISION_FP8 model; C fp32 [M][N] = relu?(A_q . W_q^T / (a_scale * w_scale) + bias) */
int cn_op_gemm_fp8(const void* a_bf16_dev, int32_t lda, const float* w_host, const float* bias_dev, float* c_dev, int32_t M,
                   int32_t N, int32_t K, float a_scale, int32_t relu, float* w_scale_out, void* stream);
/* bf16 [M][ld] -> e4m3fn bytes [M][K] at `scale` (round to nearest even, saturating at +-448): the activation quantiser */
/* Global CMVN of a padded (B, T, F) float32 batch in place: frames t < len[b] become float((double(x) - mean[f]) / std[f]) - the
 * reference's SpeechDataset arithmetic (src/data/speech_loader.py:109-115, 147-149: numpy float64 with float64 statistics, rounded to
 * float32 at collate) bit for bit; later frames (padding) are left alone.  mean / std: F doubles on the device. */
int cn_op_cmvn(float* feats_dev, const int32_t* len_dev, const double* mean_dev, const double* std_dev, int32_t B, int32_t T, int32_t F,
               void* stream);
/* The reader's collate on the device (SuperviseLoader.collate_fn, src/data/speech_loader.py:327-356; global CMVN :109-115, 147-149):
 * the utterances of an engine pass arrive packed - archive rows back to back, utterance r at row off_dev[r], len_dev[r] frames - and
 * are spread over the padded batch out_dev (rows, T, F): frames past an utterance's length are `pad`; with statistics (float64, [F])
 * a frame becomes float((double(x) - mean) / std), the dataset's arithmetic bit for bit. */
int cn_op_unpack_rows(const float* packed_dev, const int32_t* off_dev, const int32_t* len_dev, float* out_dev, int32_t rows, int32_t T,
                      int32_t F, float pad, const double* mean_dev, const double* std_dev, void* stream);
/* The same hand-over for Kaldi COMPRESSED matrices (`copy-feats --compress=true`, steps/make_fbank.sh: tokens CM / CM2 / CM3,
 * kind_dev[r] = 1 / 2 / 3; a pass may mix them).  staged_dev holds the payloads as the archive does - 16-byte global header (float
 * min_value, float range, int32 num_rows, int32 num_cols), then for kind 1 num_cols x 4 uint16 column headers and num_cols x
 * num_rows bytes column-major, for kind 2 / 3 num_rows x num_cols uint16 / uint8 row-major - payload r at BYTE offset off_dev[r], a
 * multiple of 16 (staged_dev itself 16-byte aligned).  The caller has checked num_cols == F, num_rows == len_dev[r] and the
 * payload sizes.  out_dev[r][t][:] = t < len[r] ? norm(decompress(payload r)[t][:]) : pad, the decompression in Kaldi's float32
 * arithmetic (no fused multiply-add: the bits `copy-feats` itself gives), norm as in cn_op_unpack_rows. */
int cn_op_unpack_compressed(const void* staged_dev, const int32_t* off_dev, const int32_t* len_dev, const int32_t* kind_dev,
                            float* out_dev, int32_t rows, int32_t T, int32_t F, float pad, const double* mean_dev, const double* std_dev,
                            void* stream);
/* Frame splicing and skipping behind the same hand-over (SpeechDataset.__getitem__, src/data/speech_loader.py:141-158; context_feat /
 * skip_feat, src/data/feat_op.py:4-31): float32 source rows, utterance r = len_dev[r] rows of F0 values at ROW off_dev[r] of src_dev,
 * -> out_dev (rows, T_out, (left + right + 1) * F0).  With T = len[r], Tp = T rounded up to a multiple of skip (skip > 1; else T) and
 * n_out = min(skip > 1 ? Tp / skip : T, T_out):
 *   out[r][t][k * F0 + f] = pad for t >= n_out; otherwise, with s = clamp(t * skip + k - left, 0, Tp - 1),
 *                         = s < T ? norm(src[off[r] + s][f]) : 0.0f     (the rows the dataset appends are zeros AFTER the CMVN)
 * norm as in cn_op_unpack_rows (float64, one rounding; statistics over the F0 source columns), the identity without statistics.
 * No row at or behind len[r] of an utterance is read, so the source may also be a padded, already normalised batch (rows, T0, F0)
 * with off[r] = r * T0 and no statistics.  left = right = 0, skip <= 1 is cn_op_unpack_rows.
 * Refused (-1, out_dev untouched): null pointers, a mean without a std, rows / T_out / F0 < 1, rows > 65535, left / right outside
 * [0, 64], skip outside [0, 64] (0 and 1 both keep every frame), (left + right + 1) * F0 > 12288 (a spliced row must fit the
 * kernel's 48 KB of LDS), rows * T_out * spliced width or T_out * skip beyond 2^31 - 1. */
int cn_op_splice_rows(const float* src_dev, const int32_t* off_dev, const int32_t* len_dev, float* out_dev, int32_t rows, int32_t T_out,
                      int32_t F0, int32_t left, int32_t right, int32_t skip, float pad, const double* mean_dev, const double* std_dev,
                      void* stream);
/* host side of the same reader: n byte ranges (an utterance's rows in the memory map of its archive) copied back to back into a
 * staging buffer (dst + dst_offsets[i]) by one GIL-free call; threads > 1 deals them over that many host threads */
int cn_host_gather(void* dst, const uint64_t* src_ptrs, const uint64_t* dst_offsets, const uint64_t* nbytes, int32_t n, int32_t threads);
/* ---- FLAC input (RFC 9639, 16-bit streams): frames indexed on the host, decoded on the device --------------------
 * cn_host_flac_index: the exact frame index of the audio bytes of a stream (from its first frame to the end of the file) whose
 * STREAMINFO says (rate, channels, bits) - one linear, GIL-free pass.  From the start of the current frame a running CRC-16
 * (0x8005, initial 0, MSB first) is kept; a later position becomes the next frame start only when a complete header stands there -
 * sync, valid codes, reserved bits 0, the expected next frame number (variable block size: sample number), explicit block size /
 * rate, a matching CRC-8 (0x07), the stream's blocking strategy - AND the two bytes in front of it equal the running CRC-16 of
 * everything before them.  A sync pattern inside a payload is stepped over.  The last frame ends at nbytes, where its own CRC-16
 * is checked.  out: `capacity` rows of three int32 - byte offset, byte length, first sample - or NULL to count; *frames, *samples:
 * what was found.  0, or (error set, *bad_offset: where) -2 no chain of frames with matching CRCs reaches the end (the offset of
 * the frame whose end was not found), -3 a frame whose rate, channels or sample size differ from STREAMINFO's, -5 more than
 * `capacity` frames, -6 offsets or samples beyond 2^31 - 1.
 * cn_op_flac_decode: the frames of a pass -> interleaved little-endian int16 PCM, on the device.  staged_dev: the files' bytes,
 * utterance r's at a 16-byte-aligned offset (cn_host_gather's layout); table_dev [frames][4] int32: per frame its byte offset in
 * staged_dev, byte length, utterance and first sample, in any order; utt_dev [3][utts] int32: channels, samples per channel, byte
 * offset of the utterance's PCM in pcm_dev (even; the packed reader uses multiples of 16).  Sample j of channel c of utterance r is
 * written to pcm_dev + offset[r] + 2 * (j * channels + c): the data chunk of a WAV file holding the same samples, which
 * cn_op_fbank_packed and cn_op_wave_resample read as they are.  Nothing else of pcm_dev is written.  frame_words: the largest
 * cn_flac_frame_words(channels, block size) of the pass (it sizes the scratch); max_channels: the largest channel count.
 * scratch_dev: cn_flac_scratch_bytes(frames, frame_words) bytes of the caller's, or NULL - the call then allocates them and
 * returns when the stream has drained.  status_dev: one int32, 0 after a pass whose frames all decoded; a frame that fails - a
 * table entry outside the buffers, a header that does not parse, a block that does not fit the utterance or frame_words, a
 * bitstream that leaves the frame's bytes or does not end on the footer - writes no PCM and leaves its index + 1 there (the
 * largest).  Every read is bounded by the frame's byte span, every write by the utterance's samples. */
int cn_host_flac_index(const void* audio, int64_t nbytes, int32_t rate, int32_t channels, int32_t bits, int32_t* out, int64_t capacity,
                       int64_t* frames, int64_t* samples, int64_t* bad_offset);
/* the frames' CRC-16 (polynomial 0x8005, initial value 0, MSB first) of nbytes bytes; host only (tools that write FLAC) */
int32_t cn_host_flac_crc16(const void* data, int64_t nbytes);
int64_t cn_flac_frame_words(int32_t channels, int32_t block_size);
int64_t cn_flac_scratch_bytes(int32_t frames, int64_t frame_words);
int cn_op_flac_decode(const void* staged_dev, int64_t staged_bytes, const int32_t* table_dev, int32_t frames, const int32_t* utt_dev,
                      int32_t utts, int32_t max_channels, int64_t frame_words, void* pcm_dev, int64_t pcm_bytes, int32_t* status_dev,
                      void* scratch_dev, int64_t scratch_bytes, void* stream);
int cn_op_quantize_fp8(const void* src_bf16_dev, int32_t ld, void* dst_dev, int32_t M, int32_t K, float scale, void* stream);
/* generator tail of the autoregressive step (src/models/transformer.py:48-51, 199-200): log_softmax(logits / T) and its per-row
 * top-k (sorted descending, ties: lower index) in one pass; the logits [M][V] are left untouched */
int cn_op_logsoftmax_topk(const float* logits, int32_t M, int32_t V, float temperature, int32_t k, int32_t* idx, float* val,
                          void* stream);
/* LM shallow fusion tails (src/models/transformer.py:190-192, 208-209), rows of V fp32 logits:
 * cn_op_logsoftmax_fuse_topk: top-k (1 <= k <= min(32, V), V <= 8192) over V of log_softmax(att / T) + fl32(w * log_softmax(lm)),
 *   float32 with one rounding per operation, sorted descending (ties: lower index);
 * cn_op_logsoftmax_gather: out [M][k] = log_softmax(logits) at cand [M][k] (k <= 256, V <= 16384; a candidate outside [0, V): -inf) */
int cn_op_logsoftmax_fuse_topk(const float* att, const float* lm, int32_t M, int32_t V, float temperature, float w, int32_t k,
                               int32_t* idx, float* val, void* stream);
int cn_op_logsoftmax_gather(const float* logits, int32_t M, int32_t V, const int32_t* cand, int32_t k, float* out, void* stream);
/* The step kernels of the AST beam search one at a time (cn_decode_ast runs them inside its loop).
 * cn_op_ast_gather_attn: single-query attention of n rows over gathered keys, d = 64 * H (head h at columns 64h..), elements of
 *   the precision's type.  mode 0 (decoder self-attention over the KV cache k / v [pos][slots][d]): key j of row r is cache row
 *   (j, anc[r][j]), allowed iff keyok[r][j] (tables [n][table_stride]); q rows hold the fused projection Q | K | V (ldq >= 3d) and
 *   append_pos >= 0 also writes row r's K | V to cache row (append_pos, slot r) and reads key append_pos from q's row.  mode 1
 *   (source attention): k / v point at the K and V columns of rows [B * nkeys] of stride 2d; key j of row r is row
 *   utt[r] * nkeys + j, allowed iff keymask[utt[r]][j].  Masked keys score float32 min (a row without an allowed key averages all). */
int cn_op_ast_gather_attn(int32_t precision, int32_t mode, const void* q, int32_t ldq, void* k, void* v, void* o, int32_t ldo, int32_t n,
                          int32_t H, int32_t nkeys, int32_t slots, int32_t d, int32_t table_stride, const int32_t* anc, const uint8_t* keyok,
                          const int32_t* utt, const uint8_t* keymask, float scale, int32_t append_pos, void* stream);
/* cn_op_ast_gather_attn_rows: mode 0 with a position per row (the LM step of the CTC prefix beam): row r has pos[r] + 1 keys, key j
 *   is cache row rowid[r][j] of k / v [rows][d] (table [n][table_stride], table_stride >= max_keys), every key allowed; the row's own
 *   K | V are written to cache row rowid[r][pos[r]] and key pos[r] is read from q's row.  A row with stay[r] != 0 or a position
 *   outside [0, max_keys) reads and appends nothing and gets a zero output row. */
int cn_op_ast_gather_attn_rows(int32_t precision, const void* q, int32_t ldq, void* k, void* v, void* o, int32_t ldo, int32_t n, int32_t H,
                               int32_t d, int32_t table_stride, int32_t max_keys, const int32_t* rowid, const int32_t* pos,
                               const int32_t* stay, float scale, void* stream);
/* CTC side (src/utils/ctc_prefix.py): prepare masks logp [B][Tp][V] in place (frames with keymask 0: logzero, blank 0) and writes
 * the initial states r0 [B][Tp][2]; prefix scores the K candidates cand [n][K] of n prefixes of out_len tokens (0 <= out_len <= Tp)
 * -> score [n][K] and states r_new [n * K][Tp][2]; prev_ref[h] >= 0 takes row prev_ref[h] of r_prev, < 0 the initial state of
 * utterance -1 - prev_ref[h]. */
int cn_op_ast_ctc_prepare(float* logp, const uint8_t* keymask, float* r0, int32_t B, int32_t Tp, int32_t V, int32_t blank, void* stream);
int cn_op_ast_ctc_prefix(const float* logp, const float* r0, const float* r_prev, float* r_new, const int32_t* utt, const int32_t* last_tok,
                         const int32_t* cand, const int32_t* prev_ref, float* score, int32_t n, int32_t K, int32_t Tp, int32_t V,
                         int32_t blank, int32_t eos, int32_t out_len, void* stream);
/* Beam bookkeeping on the device state of cn_decode_ast, both parities of every double-buffered array passed separately
 * (S = B * bw slots, L tokens per slot): tok / anc int32 [S][L], keyok uint8 [S][L], len / valid / ctc_ref int32 [S], score double
 * [S], ctc_prev float [S]; cur_tok / utt int32 [S]; live int32 [1].  init fills parity cur; update reads parity cur and this
 * step's candidates (idx / att / ctc / lm [S][K]) and writes parity cur ^ 1.  1 <= bw <= K <= 32. */
int cn_op_ast_beam_init(int32_t* tok0, int32_t* tok1, int32_t* anc0, int32_t* anc1, uint8_t* keyok0, uint8_t* keyok1, int32_t* len0,
                        int32_t* len1, double* score0, double* score1, int32_t* valid0, int32_t* valid1, int32_t* ctc_ref0, int32_t* ctc_ref1,
                        float* ctc_prev0, float* ctc_prev1, int32_t* cur_tok, int32_t* utt, int32_t* live, int32_t cur, int32_t B, int32_t bw,
                        int32_t L, int32_t sos, int32_t pad, void* stream);
int cn_op_ast_beam_update(int32_t* tok0, int32_t* tok1, int32_t* anc0, int32_t* anc1, uint8_t* keyok0, uint8_t* keyok1, int32_t* len0,
                          int32_t* len1, double* score0, double* score1, int32_t* valid0, int32_t* valid1, int32_t* ctc_ref0,
                          int32_t* ctc_ref1, float* ctc_prev0, float* ctc_prev1, int32_t* cur_tok, int32_t* utt, int32_t* live,
                          const int32_t* idx, const float* att, const float* ctc, const float* lm, int32_t cur, int32_t pos, int32_t bw,
                          int32_t K, int32_t L, int32_t eos, int32_t sos, int32_t pad, int32_t use_ctc, int32_t use_lp, int32_t use_lm,
                          float w, float u, float lw, double lp, int32_t B, void* stream);

/* The two kernels of cn_nat_lm_finish one at a time.  cn_op_nat_lm_fuse_topk: slot s = b * bw + j of B * bw slots takes
 * att [B][U][V] row (b, step) - log-probabilities, NOT normalised again; all zero when zlen && step >= zlen[b] - plus
 * fl32(w * log_softmax(lm [B * bw][V] row s)) and writes its k best (1 <= k <= min(32, V), V <= 8192; sorted descending, ties: lower
 * index) to idx / val [B * bw][k]; slots of an utterance with step > last[b] are skipped (last / zlen [B] may be NULL).
 * cn_op_nat_beam_update: one step of the bookkeeping (src/models/cassnat.py:613-636) on double-buffered state (S = B * bw slots
 * of L tokens: tok / anc int32 [S][L], keyok uint8 [S][L], score double [S]; cur_tok int32 [S]): reads parity cur and the step's
 * candidates idx / val [S][bw], writes parity cur ^ 1; one live beam per utterance at step 0, bw afterwards; an utterance with
 * step > last[b] carries its beams.  1 <= bw <= 16, step <= L - 2. */
int cn_op_nat_lm_fuse_topk(const float* att, const float* lm, const int32_t* last, const int32_t* zlen, int32_t B, int32_t U, int32_t V,
                           int32_t bw, int32_t step, float w, int32_t k, int32_t* idx, float* val, void* stream);
int cn_op_nat_beam_update(int32_t* tok0, int32_t* tok1, int32_t* anc0, int32_t* anc1, uint8_t* keyok0, uint8_t* keyok1, double* score0,
                          double* score1, int32_t* cur_tok, const int32_t* idx, const float* val, const int32_t* last, int32_t cur,
                          int32_t step, int32_t bw, int32_t L, int32_t pad, int32_t use_lp, double lp, int32_t B, void* stream);

/* The kernels of cn_ctc_beam_lm's loop one at a time (ctc_lm.hip); every array is the caller's, on the device.  S = B * W slots.
 * cn_op_ctc_lm_frame: iteration `iter` of the frame step on given log-posteriors logp [B][Tp][V], pruned labels top_idx [B][Tp][P],
 * LM rows lmrow [S][V] and schedule frames [B][Tp] / count [B].  Beam state, updated in place: pb / pnb / sctc / slm double [S],
 * len / last int32 [S] (last -1: empty), nb int32 [B]; LM tables written for the next step: tok / pos / parent / stay int32 [S],
 * rowid_nxt [S][Lt] from rowid_cur [S][Lt] (the parent's ids, plus (iter + 1) * S + slot for an appended label); back-pointers
 * hist_parent uint8 / hist_tok int32 [B][hist_stride][W] at row iter.  An utterance with iter >= count[b] only sets stay.
 * 1 <= W <= 32, 0 <= P <= 32, Lt >= iter + 2, iter < hist_stride.
 * cn_op_ctc_lm_rows: nxt[s] = stay[s] ? prv[parent[s]] : fresh[s] over [S][V] rows; slots of an utterance with iter >= count[b]
 * are skipped (count may be NULL). */
int cn_op_ctc_lm_frame(double* pb, double* pnb, double* sctc, double* slm, int32_t* len, int32_t* last, int32_t* nb, int32_t* tok,
                       int32_t* pos, int32_t* parent, int32_t* stay, const int32_t* rowid_cur, int32_t* rowid_nxt, uint8_t* hist_parent,
                       int32_t* hist_tok, const float* logp, const int32_t* top_idx, const float* lmrow, const int32_t* frames,
                       const int32_t* count, int32_t B, int32_t Tp, int32_t V, int32_t W, int32_t P, int32_t blank, int32_t sos,
                       int32_t iter, int32_t Lt, int32_t hist_stride, double lp, double lm_weight, void* stream);
int cn_op_ctc_lm_rows(const float* fresh, const float* prv, float* nxt, const int32_t* parent, const int32_t* stay, const int32_t* count,
                      int32_t iter, int32_t slots, int32_t W, int32_t V, void* stream);

/* ---- ARPA n-gram model: the ESA ranker `rank_model: n-gram` (ngram.hip; models/ngram.py owns the tables) ---------------------
 * The score of a row of word-piece ids is log10 P(w_1 .. w_m </s> | <s>) of the words its pieces spell, with textbook ARPA back-off:
 * the history of a word is the last c = min(order - 1, words so far + 1) ids, starting with <s>; p is the probability of the longest
 * k-gram (k = c + 1 .. 1) of the model that ends in the word, and the back-off weights of the j-grams made of the last j history ids
 * are added for j = k .. c in that order (an absent n-gram or weight adds nothing).  float32 throughout: a word's score is summed in
 * that order, the row's score is the sum of the word scores in word order, </s> last.
 * Hashing.  A word's key is H(bytes) = sum (byte_i + 1) * P^(n - 1 - i) mod 2^64 with P = 0x9E3779B97F4A7C15, so that
 * H(ab) = H(a) * P^len(b) + H(b): a piece of the vocabulary contributes the pair (H(body), P^len(body)) and a flag "begins with a
 * separator" (U+2581 or ASCII white space, a leading run only; the body may be empty).  An n-gram's key mixes its order and ids.
 * Look-ups compare the 64-bit key alone (key_mask keeps the low hash_bits of every key: a test's way to make keys collide).
 * Tables: open addressing with linear probing, power-of-two slot counts, at most half full.  word_ids < 0 and gram_prob = +infinity
 * mark an empty slot.  Every pointer of a desc is a device pointer for cn_op_ngram_score and a host pointer for the host entries. */
typedef struct cn_ngram_desc {
    const uint64_t* word_keys; /* [word_slots] */
    const int32_t* word_ids;   /* [word_slots] */
    int64_t word_slots;
    const uint64_t* gram_keys; /* [gram_slots] */
    const float* gram_prob;    /* [gram_slots] */
    const float* gram_bo;      /* [gram_slots] */
    int64_t gram_slots;
    const uint64_t* piece_hash; /* [vocab] H(body) */
    const uint64_t* piece_pow;  /* [vocab] P^len(body) */
    const uint8_t* piece_starts; /* [vocab] 1: the piece begins with a separator */
    int32_t vocab;
    int32_t order;             /* 1 .. 8 */
    int32_t bos, eos, unk;     /* word ids of <s>, </s>, <unk> */
    int32_t reserved0;
    uint64_t key_mask;
    int64_t reserved[6];
} cn_ngram_desc;
int32_t cn_ngram_desc_size(void);
/* Host only, no GPU involved.  cn_ngram_counts reads the \data\ header of an ARPA text: counts[0] = order (1 .. 8, else refused),
 * counts[k] = the `ngram k=` value.  cn_ngram_parse reads the whole text into tables the caller allocated (word_slots / gram_slots:
 * powers of two, at least 2 * (counts[1] + 1) and 2 * (sum of the counts + 1)); word ids are the positions in the 1-gram section, a
 * file without <unk> gets one more id with probability -100.  info[0..8) = order, ids, entries, entries whose prefix or suffix
 * (n - 1)-gram is not in the file, the ids of <s>, </s>, <unk>, and 1 when the file has <unk>.  Refused with the line's number
 * in the message: a section whose line count differs from its `ngram k=` line, a malformed line, a missing <s> or </s>, two entries
 * with the same key.  cn_ngram_hash: H and P^len of n byte strings, string i = bytes[off[i], off[i + 1]). */
int cn_ngram_counts(const void* text, int64_t bytes, int64_t* counts);
int cn_ngram_parse(const void* text, int64_t bytes, int32_t hash_bits, uint64_t* word_keys, int32_t* word_ids, int64_t word_slots,
                   uint64_t* gram_keys, float* gram_prob, float* gram_bo, int64_t gram_slots, int64_t* info);
int cn_ngram_hash(const void* bytes, const int64_t* off, int32_t n, uint64_t* h, uint64_t* pw);
/* Scores of `rows` rows of tok [rows][stride] (row r: its first len[r] ids, clamped to [0, stride]); ids equal to drop_id are left
 * out, an id outside [0, vocab) is never used as an index: it stands for a piece that begins a word no model holds.  score [rows]
 * float32; nothing else is written.  cn_ngram_score_host runs on the host with host pointers; cn_op_ngram_score is one wave per row
 * on the device, stateless, ordered on `stream`; the two share one scoring core and agree bit for bit.  Refused without a launch
 * (-1): a null pointer, rows or stride < 1, vocab < 0, an order outside 1 .. 8, a slot count that is no power of two. */
int cn_ngram_score_host(const cn_ngram_desc* desc, const int32_t* tok, int32_t stride, const int32_t* len, int32_t rows,
                        int32_t drop_id, float* score);
int cn_op_ngram_score(const cn_ngram_desc* desc, const int32_t* tok_dev, int32_t stride, const int32_t* len_dev, int32_t rows,
                      int32_t drop_id, float* score_dev, void* stream);
#ifdef __cplusplus
}
#endif
#endif
