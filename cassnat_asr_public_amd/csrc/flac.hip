// FLAC (RFC 9639, 16-bit streams) decoded on the device: the packed reader stages the files' frames as they are - about half the
// bytes of the 16-bit PCM - with the frame table the host index found (flac_format.h: exact, every frame's CRC-16 checked there), and
// these kernels write the interleaved int16 PCM exactly as the data chunk of a WAV file would hold it, so that fbank_packed / the
// resampler read it unchanged.  Frames are independent: nothing walks an utterance.  Three launches over the pass's frames
// (flac_decode.h holds the per-frame routines, the same code the host checker runs):
//   entropy   one lane per frame: header, subframe headers, warm-up samples and Rice / escaped residuals -> int32 words in the
//             scratch.  The bitstream is serial, so this is the long pole: about one bit-reader step per sample; the frame's bytes
//             are fetched straight through L2 (a lane walks its own frame front to back, 64 distinct streams per wave).
//   restore   one lane per (frame, channel): the fixed / LPC recurrence in place, reading back the words it wrote (order + 1 loads
//             and order 64-bit multiply-adds per sample).
//   output    one workgroup per frame: wasted bits, left/side - side/right - mid/side undone, coalesced int16 stores.
// Scratch layout: the words of the 64 frames of a group are interleaved - word k of lane l at (group * frame_words + k) * 64 + l - so
// that lanes at similar positions of their frames write neighbouring addresses; a frame takes flac_frame_words(channels, block size)
// words, frame_words is the pass's largest.  4 bytes written and read twice per sample, 2 bytes out.
// Bounds: reads stay inside the frame's byte span (itself checked against staged_bytes), word indices inside frame_words, PCM
// stores inside the utterance's samples (checked against pcm_bytes).  A frame that fails any check writes no PCM and leaves its
// index + 1 in the status word (the largest failing one wins).
#include "flac_decode.h"
#include "kernels.h"

struct FlacParams {
    const unsigned char* staged;
    long long staged_bytes;
    const int* table;  // [frames][4]: byte offset, byte length, utterance, first sample
    int frames;
    const int* utt;    // [3][utts]: channels, samples per channel, byte offset of the PCM
    int utts;
    int* scratch;
    long long frame_words;
    unsigned char* pcm;
    long long pcm_bytes;
    int* status;
};

__device__ inline int* flac_words(const FlacParams& p, int f) { return p.scratch + ((long long)(f >> 6) * p.frame_words << 6) + (f & 63); }

__global__ __launch_bounds__(64) void flac_entropy_kernel(FlacParams p) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= p.frames) return;
    int* w = flac_words(p, f);
    const long long off = p.table[4 * f], len = p.table[4 * f + 1], first = p.table[4 * f + 3];
    const int u = p.table[4 * f + 2];
    int bad = 7;  // a table entry that points outside the pass
    w[0] = 0;
    if (off >= 0 && len > 0 && off + len <= p.staged_bytes && u >= 0 && u < p.utts) {
        const long long C = p.utt[u], n = p.utt[p.utts + u], at = p.utt[2 * p.utts + u];
        if (C >= 1 && C <= 8 && first >= 0 && first < n && at >= 0 && !(at & 1) && at + 2 * C * n <= p.pcm_bytes)
            bad = flac_entropy_frame(p.staged + off, len, (int)C, n - first, p.frame_words, w, 64, false);
    }
    if (bad) atomicMax(p.status, f + 1);
}

__global__ __launch_bounds__(64) void flac_restore_kernel(FlacParams p) {
    const int f = blockIdx.x * 64 + threadIdx.x, c = blockIdx.y;
    if (f >= p.frames) return;
    int* w = flac_words(p, f);
    if (w[0] != 1 || c >= w[3 * 64]) return;
    flac_restore_channel(w, 64, c);
}

__global__ __launch_bounds__(256) void flac_output_kernel(FlacParams p) {
    const int f = blockIdx.x;
    const int* w = flac_words(p, f);
    if (w[0] != 1) return;
    const int bs = w[1 * 64], C = w[3 * 64], u = p.table[4 * f + 2];
    const long long first = p.table[4 * f + 3];
    short* out = reinterpret_cast<short*>(p.pcm + p.utt[2 * p.utts + u]) + first * C;  // (the entropy step checked all of these)
    for (int k = threadIdx.x; k < bs * C; k += 256) out[k] = (short)flac_output_sample(w, 64, k % C, k / C);
}

long long flac_scratch_bytes(int frames, long long frame_words) { return (long long)((frames + 63) / 64) * 64 * frame_words * 4; }

int launch_flac_decode(const unsigned char* staged, long long staged_bytes, const int* table, int frames, const int* utt, int utts,
                       int max_channels, long long frame_words, unsigned char* pcm, long long pcm_bytes, int* status, int* scratch,
                       hipStream_t s) {
    FlacParams p = {};
    p.staged = staged;
    p.staged_bytes = staged_bytes;
    p.table = table;
    p.frames = frames;
    p.utt = utt;
    p.utts = utts;
    p.scratch = scratch;
    p.frame_words = frame_words;
    p.pcm = pcm;
    p.pcm_bytes = pcm_bytes;
    p.status = status;
    CN_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int), s));
    const unsigned groups = (unsigned)((frames + 63) / 64);
    hipLaunchKernelGGL(flac_entropy_kernel, dim3(groups), dim3(64), 0, s, p);
    hipLaunchKernelGGL(flac_restore_kernel, dim3(groups, (unsigned)max_channels), dim3(64), 0, s, p);
    hipLaunchKernelGGL(flac_output_kernel, dim3((unsigned)frames), dim3(256), 0, s, p);
    CN_HIP_CHECK(hipGetLastError());
    return 0;
}
