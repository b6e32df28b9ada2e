// dmf_attr_criteria.h — the three criteria of the multi-attribute profile, each stated once, for the device
// (at_multi_count_kernel of dmf_attr.hip) and for the host compiler (tests/attr_criteria_check.cpp).  A criterion is a function of
// what the root pass accumulated for a 4-connected component S of {q >= t} — its pixel count, the extremes of its columns and
// rows, the sum of q and of q^2 over its pixels — and of a whole-number threshold tau.  Unsigned 64-bit, no division, no float.
//
// OVERFLOW (the one statement of it).  size = |S| >= 1.
//   area      size >= tau.                                          size, tau < 2^31.
//   diagonal  w^2 + h^2 >= tau^2, w and h the side lengths in pixels of S's bounding box.  w, h, tau < 2^31 (H W < 2^31, so each
//             side is), so each square is < 2^62 and the sum is < 2^63.
//   std       size sum_q2 - sum_q^2 >= tau^2 size^2: the population variance of q over S is >= tau^2, multiplied through by
//             size^2.  With size <= H W <= 2^22 (DMF_ATTR_STD_PIXELS_MAX), q <= 255 < 2^8 and tau <= 255:
//               size sum_q2  <= 2^22 (2^22 2^16) = 2^60        sum_q^2 <= (2^22 2^8)^2 = 2^60        tau^2 size^2 < 2^16 2^44 = 2^60
//             and the left side is >= 0 by Cauchy-Schwarz ((sum q)^2 <= size sum q^2), so the unsigned subtraction does not wrap.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define DMF_ATTR_HD __host__ __device__
#else
#define DMF_ATTR_HD
#endif

namespace dmf {

DMF_ATTR_HD inline bool attr_crit_area(uint32_t size, uint32_t tau) { return size >= tau; }

// box: the smallest and largest column and row of S, inclusive
DMF_ATTR_HD inline bool attr_crit_diagonal(int32_t xmin, int32_t xmax, int32_t ymin, int32_t ymax, uint32_t tau) {
  const uint64_t w = (uint64_t)((int64_t)xmax - xmin + 1), h = (uint64_t)((int64_t)ymax - ymin + 1);
  return w * w + h * h >= (uint64_t)tau * tau;
}

DMF_ATTR_HD inline bool attr_crit_std(uint32_t size, uint64_t sum_q, uint64_t sum_q2, uint32_t tau) {
  const uint64_t s = size;
  return s * sum_q2 - sum_q * sum_q >= (uint64_t)tau * tau * s * s;
}

}  // namespace dmf
