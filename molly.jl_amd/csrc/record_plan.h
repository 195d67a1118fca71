// record_plan.h — at which steps of a run the recorder fires, for which channels, and whether the records fit.  Host-only arithmetic on plain
// values: no HIP header, nothing of the engine (tests/host/record_plan_check.cpp runs it alone), no state, no allocation, everything by value.
//
// A channel c with interval every[c] > 0 records at every step s with s % every[c] == 0 (apply_loggers!, loggers.jl:44-56: step numbering is
// global, so a run continued in chunks continues one history).  A run (first, n) takes the steps first + 1 … first + n: the step `first` itself
// belongs to the caller (the reference's initial apply_loggers! is mhip_record_now).
//
//   rec_next_step()   the first step >= s at which any channel fires (REC_NEVER: all channels off, or none up to the largest step number)
//   rec_mask()        the channels that fire at step s, bit c for channel c
//   rec_count()       how many records each channel makes in the run (first, n)
//   rec_fits()        whether those records fit the free capacity of every channel that is on
#pragma once
#include <algorithm>
#include <cstdint>

namespace mhip {

constexpr int REC_CHANNELS = 4;                  // MHIP_REC_KE, MHIP_REC_PE, MHIP_REC_COORDS, MHIP_REC_VELOCITIES
constexpr int64_t REC_NEVER = INT64_MAX;

struct RecEvery { int32_t every[REC_CHANNELS]; };      // 0: the channel is off
struct RecCount { int64_t n[REC_CHANNELS]; };

inline bool rec_any(RecEvery e) {
    for (int c = 0; c < REC_CHANNELS; ++c) if (e.every[c] > 0) return true;
    return false;
}

// the multiples of k > 0 in (lo, hi], lo <= hi, any sign (floor division)
inline int64_t rec_floor_div(int64_t a, int64_t k) { return a / k - ((a % k != 0 && a < 0) ? 1 : 0); }
inline int64_t rec_multiples_in(int64_t lo, int64_t hi, int64_t k) { return hi <= lo ? 0 : rec_floor_div(hi, k) - rec_floor_div(lo, k); }

inline int rec_mask(RecEvery e, int64_t s) {
    int m = 0;
    for (int c = 0; c < REC_CHANNELS; ++c) if (e.every[c] > 0 && s % e.every[c] == 0) m |= 1 << c;
    return m;
}

inline int64_t rec_next_step(RecEvery e, int64_t s) {
    int64_t best = REC_NEVER;
    for (int c = 0; c < REC_CHANNELS; ++c) {
        const int64_t k = e.every[c];
        if (k <= 0) continue;
        const int64_t q = rec_floor_div(s, k), at = q * k;      // the multiple at or below s
        if (at == s) return s;
        if (q >= INT64_MAX / k) continue;                        // the next multiple is beyond the largest step number
        best = std::min(best, at + k);
    }
    return best;
}

inline RecCount rec_count(RecEvery e, int64_t first, int64_t n) {
    RecCount r{};
    const int64_t last = n > 0 && first <= INT64_MAX - n ? first + n : (n > 0 ? INT64_MAX : first);
    for (int c = 0; c < REC_CHANNELS; ++c) r.n[c] = e.every[c] > 0 ? rec_multiples_in(first, last, e.every[c]) : 0;
    return r;
}

// used[c] records are held, capacity[c] is the room of the channel's buffer
inline bool rec_fits(RecEvery e, int64_t first, int64_t n, RecCount used, RecCount capacity) {
    const RecCount add = rec_count(e, first, n);
    for (int c = 0; c < REC_CHANNELS; ++c)
        if (e.every[c] > 0 && add.n[c] > capacity.n[c] - std::min(used.n[c], capacity.n[c])) return false;
    return true;
}

}  // namespace mhip
