/* C ABI of the energy voice-activity detector (bin/make_segments): a companion of cassnat_hip.h.  Exported by the same libraries and
 * bound by the same parser (cassnat_asr_public_amd/abi.py: VAD_FUNCTIONS); one declaration per entry point, plain arguments, no struct. */
#ifndef CASSNAT_HIP_VAD_H
#define CASSNAT_HIP_VAD_H
#include "cassnat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* partial sums the device keeps per recording behind the thresholds (cn_op_vad_decide: thr_dev) */
#define CN_VAD_PARTS 64

/* ---- frame energy (vad.hip, vad_frames.h; DESIGN.md 7p defines the values) ---------------------------------------------------------------
 * Not in the reference.  No model handle.  The samples are little-endian int16 as a WAV `data` chunk holds them, at the file's own
 * rate, `channels` (1 .. 8) interleaved; row r is a run of samples[r] sample frames at BYTE offset off[r] of `staged`, a multiple of 16
 * (the layout cn_host_gather and cn_op_fbank_packed use).  Nothing outside [0, staged_bytes) is read: a row that reaches outside is cut
 * to the whole sample frames that lie inside, and no byte in front of a row or behind its last sample frame is read either (any even
 * offset is read correctly; a row whose offset is negative or odd has no frames).
 * Frames are Kaldi's snip-edges frames of `channel`: frame t covers the sample frames [t shift, t shift + N), T = 1 + (n - N) / shift
 * for n >= N else 0, and at most max_frames (which sizes the launch).  Per frame, exactly: S1 = sum x, S2 = sum x^2,
 * num = N S2 - S1^2 (remove_dc) or S2; then E = double(num) / N (one rounding) or double(num), e = log(max(E, 2^-23)).
 * Frame t of row r is written at index out_off[r] + t of num and of e; nothing else of either is written.
 * cn_op_frame_energy: every pointer a device pointer (staged 16-byte aligned), one launch on `stream`, nothing allocated, nothing
 * waited for.  cn_frame_energy_host: the same definition, serial, host pointers, no GPU call; num agrees in every bit, e to what two
 * 1-ulp logarithms differ.
 * Refused before anything runs (-1, cn_last_error): a null pointer, rows <= 0 (or > 65535), N outside 1 .. 2048, shift < 1, channels
 * outside 1 .. 8, channel outside [0, channels), max_frames < 1.
 *
 * ---- decision: Kaldi's ComputeVadEnergy ------------------------------------------------------------------------------------------------
 * Recording i holds the frames e[rec_off[i] .. rec_off[i] + T), T = max(rec_frames[i], 0).  thr = thr0 + mean_scale * ((sum e) / T), or
 * thr0 when mean_scale == 0 or T == 0; raw[t] = e[t] > thr; dec[t] = double(#raw over W) >= double(#W) * proportion over the window
 * W = [t - context, t + context] cut to [0, T); context 0 .. 64; all in double.  dec (one byte per frame, 0 / 1) lies at the frames'
 * own indices; thr[i] is recording i's threshold.
 * cn_op_vad_decide: thr_dev holds recs * (1 + CN_VAD_PARTS) doubles - the thresholds first, behind them the partial sums of the
 * two-level mean (CN_VAD_PARTS contiguous strips per recording, each summed in a fixed order, then added from the first to the last: no
 * atomics, the same bits in every run).  Three launches on `stream`, nothing allocated, nothing waited for.
 * cn_vad_decide_host: serial, adds from the first frame to the last; thr holds recs doubles.  dec agrees wherever no e[t] lies
 * within the two sums' rounding of thr; thr within |mean_scale| (T + 4) 2^-52 max(1, max|e|).
 * Refused (-1): a null pointer, recs <= 0 (or > 65535), context outside 0 .. 64. */
int cn_op_frame_energy(const void* staged_dev, int64_t staged_bytes, const int32_t* off_dev, const int32_t* samples_dev,
                       const int32_t* out_off_dev, int32_t rows, int32_t N, int32_t shift, int32_t channels, int32_t channel,
                       int32_t remove_dc, int32_t max_frames, int64_t* num_dev, double* e_dev, void* stream);
int cn_frame_energy_host(const void* staged, int64_t staged_bytes, const int32_t* off, const int32_t* samples, const int32_t* out_off,
                         int32_t rows, int32_t N, int32_t shift, int32_t channels, int32_t channel, int32_t remove_dc, int32_t max_frames,
                         int64_t* num, double* e);
int cn_op_vad_decide(const double* e_dev, const int32_t* rec_off_dev, const int32_t* rec_frames_dev, int32_t recs, double thr0,
                     double mean_scale, int32_t context, double proportion, double* thr_dev, uint8_t* dec_dev, void* stream);
int cn_vad_decide_host(const double* e, const int32_t* rec_off, const int32_t* rec_frames, int32_t recs, double thr0, double mean_scale,
                       int32_t context, double proportion, double* thr, uint8_t* dec);

#ifdef __cplusplus
}
#endif
#endif
