/* C ABI of the feature-archive writer (bin/make_fbank): a companion of cassnat_hip.h.  Exported by the same libraries and bound by the
 * same parser (cassnat_asr_public_amd/abi.py: FEATS_FUNCTIONS); one declaration per entry point, plain arguments, no struct. */
#ifndef CASSNAT_HIP_FEATS_H
#define CASSNAT_HIP_FEATS_H
#include "cassnat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Kaldi matrix compression on the device (feats.hip, feats_compress.h; DESIGN.md 7n defines the bytes) ---------------------------
 * Not in the reference, whose recipes take feats.scp and cmvn.ark from Kaldi's make_fbank.sh / compute-cmvn-stats.  No model handle.
 * The batch: float32 (rows, Tmax, F), padded; utterance r holds T = min(lens[r], Tmax) valid rows, and rows at or behind T are never
 * read.  Its payload - what an archive holds behind the `CM ` / `CM2 ` token: the 16-byte global header (float32 min, float32 range,
 * int32 rows, int32 columns), for T > 8 the F column headers of four uint16 and T * F bytes column-major (format 1), for T <= 8 T * F
 * uint16 row-major (format 2) - is written at out + out_off[r]; out_off are byte offsets, multiples of 16, which the caller lays out
 * from lens with cn_compress_feats_bytes.  Nothing else of `out` is written.
 * cn_compress_feats_bytes: 16 + 8 F + T F for T > 8, 16 + 2 T F for 0 <= T <= 8 (0 for T < 0 or F < 1).
 * status[r]: 0 fine; 1 lens[r] < 1; 2 a non-finite value among the valid rows (or a range max - min that overflows); 3 the payload
 * would not lie inside out_bytes at a multiple of 16.  A payload whose status is not 0 is not written at all.
 * cn_op_compress_feats: every pointer a device pointer (out 16-byte aligned), two launches on `stream`, nothing allocated, nothing
 * waited for.  cn_compress_feats_host: the same definition, serial, every pointer a host pointer, no GPU call - the same arithmetic
 * functions (csrc/feats_compress.h); the two agree in every byte and status word.
 * Refused before anything runs (-1, cn_last_error): a null or misaligned buffer, rows, Tmax or F < 1.
 *
 * ---- CMVN sums of what an archive holds -----------------------------------------------------------------------------------------------
 * stats (rows, 2, F) float64: per utterance and column the sum and the sum of squares over its T valid rows of
 *   - payload given: the values a reader dequantises from the payload at payload + out_off[r] (format 1 for T > 8, else format 2) -
 *     what compute-cmvn-stats would see in the archive, and a later decode from it;
 *   - payload NULL: the float32 rows of `feats` (an archive written without compression).
 * An utterance with T < 1, or whose status word (status may be NULL: all fine) is not 0, gives zeros; a payload is read only where the
 * status says cn_op_compress_feats wrote it.  No atomics: sixteen partial sums per column (row t into partial t % 16), added from the first to
 * the last - two runs give the same bits, and the host twin, which adds in the same order, gives them too.  Both lie within
 * (T - 1) * 2^-53 * sum|x| (resp. sum x^2) of the exact sums, as every order of additions does. */
int64_t cn_compress_feats_bytes(int32_t T, int32_t F);
int cn_op_compress_feats(const float* feats_dev, const int32_t* lens_dev, const int32_t* out_off_dev, int32_t rows, int32_t Tmax, int32_t F,
                         void* out_dev, int64_t out_bytes, int32_t* status_dev, void* stream);
int cn_compress_feats_host(const float* feats, const int32_t* lens, const int32_t* out_off, int32_t rows, int32_t Tmax, int32_t F, void* out,
                           int64_t out_bytes, int32_t* status);
int cn_op_feats_stats(const float* feats_dev, const void* payload_dev, const int32_t* out_off_dev, const int32_t* lens_dev,
                      const int32_t* status_dev, int32_t rows, int32_t Tmax, int32_t F, double* stats_dev, void* stream);
int cn_feats_stats_host(const float* feats, const void* payload, const int32_t* out_off, const int32_t* lens, const int32_t* status,
                        int32_t rows, int32_t Tmax, int32_t F, double* stats);

#ifdef __cplusplus
}
#endif
#endif
