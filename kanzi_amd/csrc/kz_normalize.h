// kz_normalize.h -- EntropyUtils.normalizeFrequencies (K/entropy/EntropyUtils.java:141-250) for one wave64 and a scale that is a
// parameter: the data-parallel restatement of kz_ans.hip (k_ans_enc_chunk, where the scale is fixed at 2^12), used by kz_range.hip.
// Lane L holds the symbols q * 64 + L, q = 0..3 (symbol order = (q, lane) lexicographic); wave reductions and ballot prefixes give the
// reference's sequential semantics.  total * scale must fit 32 bits (a 32 KiB chunk at scale 2^12: 2^27).
#pragma once
#include "kz_device.h"

// f[q]: the counts on entry, the scaled frequencies on return (0 where the symbol is absent); returns the alphabet size.
__device__ __forceinline__ uint32_t kz_normalize_wave(uint32_t f[4], uint32_t total, uint32_t scale) {
  const int lane = kz_lane();
  bool present[4];
  uint32_t alphabetSize = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) { present[q] = f[q] != 0; alphabetSize += (uint32_t)__popcll(kz_ballot(present[q])); }
  if (total == scale) return alphabetSize;                       // :155-162
  uint32_t sumScaled = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    if (present[q]) {
      const uint32_t sf = f[q] * scale;
      f[q] = (sf <= total) ? 1u : (sf + (total >> 1)) / total;
    }
    sumScaled += kz_wave_sum(present[q] ? f[q] : 0);
  }
  if (alphabetSize == 1) {
#pragma unroll
    for (int q = 0; q < 4; q++) if (present[q]) f[q] = scale;
    return alphabetSize;
  }
  if (sumScaled == scale) return alphabetSize;
  // idxMax = first symbol (in symbol order) holding the maximum scaled frequency (:184-185)
  uint32_t best = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) { const uint32_t v = present[q] ? f[q] : 0; best = max(best, v); }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) best = max(best, (uint32_t)__shfl_xor(best, d, 64));
  int idxMax = 256;
#pragma unroll
  for (int q = 3; q >= 0; q--) {
    const uint64_t bal = kz_ballot(present[q] && f[q] == best);
    if (bal) idxMax = q * 64 + (int)__builtin_ctzll(bal);
  }
  int delta = (int)sumScaled - (int)scale;
  const int errThr = (int)(best >> 4);
  const int mq = idxMax >> 6, ml = idxMax & 63;
  const int ad = delta < 0 ? -delta : delta;
  if (ad <= errThr) {                                            // :204-208 fast path
#pragma unroll
    for (int q = 0; q < 4; q++) if (q == mq && lane == ml) f[q] = (uint32_t)((int)f[q] - delta);
    return alphabetSize;
  }
  int adj;
  if (delta < 0) { delta += errThr; adj = errThr; } else { delta -= errThr; adj = -errThr; }
  // applied now: the slow path tests freqs[idx] <= 2 on the updated value
#pragma unroll
  for (int q = 0; q < 4; q++) if (q == mq && lane == ml) f[q] = (uint32_t)((int)f[q] + adj);
  const int inc = (delta > 0) ? -1 : 1;                          // :219-246
  delta = delta < 0 ? -delta : delta;
  int round = 0;
  while ((++round < 6) && (delta > 0)) {
    int adjustments = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const bool elig = present[q] && f[q] > 2;
      const uint64_t bal = kz_ballot(elig);
      const int pre = (int)__popcll(bal & kz_lanemask_lt());
      const int tot = (int)__popcll(bal);
      if (elig && pre < delta) f[q] = (uint32_t)((int)f[q] + inc);
      const int used = tot < delta ? tot : delta;
      adjustments += used; delta -= used;
    }
    if (adjustments == 0) break;
  }
  // freqs[idxMax] = max(freqs[idxMax] - delta, 1)  (:248)
#pragma unroll
  for (int q = 0; q < 4; q++) if (q == mq && lane == ml) { const int v = (int)f[q] - delta; f[q] = (uint32_t)(v > 1 ? v : 1); }
  return alphabetSize;
}
