// Stand-alone check of molly.jl_amd/csrc/record_plan.h (tests/test_record_plan_host.py compiles and runs it, with the address and undefined-behaviour
// sanitizers): known answers at the edges — a record at the run's last step, none in a run shorter than the interval, a record step equal to `first`
// not counted, all channels off, intervals 1 and 2^31 − 1 — then a sweep of firsts × lengths × interval quadruples × used / capacity against a
// brute-force loop over the steps.  Exit status 0 = pass.
#include <cstdio>

#include "record_plan.h"

using namespace mhip;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; if (failures < 50) { std::printf("FAIL %s:%d: %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static int n_known = 0;
static RecEvery ev(int32_t a, int32_t b, int32_t c, int32_t d) { return RecEvery{{a, b, c, d}}; }
static RecCount cnt(int64_t a, int64_t b, int64_t c, int64_t d) { return RecCount{{a, b, c, d}}; }
static void known_count(const char* what, RecEvery e, int64_t first, int64_t n, RecCount want) {
    ++n_known;
    const RecCount got = rec_count(e, first, n);
    for (int c = 0; c < REC_CHANNELS; ++c) CHECK(got.n[c] == want.n[c], "%s: channel %d makes %lld records, not %lld", what, c, (long long)got.n[c], (long long)want.n[c]);
}
static void known_next(const char* what, RecEvery e, int64_t s, int64_t want, int want_mask) {
    ++n_known;
    const int64_t got = rec_next_step(e, s);
    CHECK(got == want, "%s: next step %lld, not %lld", what, (long long)got, (long long)want);
    if (got != REC_NEVER) CHECK(rec_mask(e, got) == want_mask, "%s: mask %d, not %d", what, rec_mask(e, got), want_mask);
}

static void known_answers() {
    const int32_t BIG = 2147483647;      // 2^31 − 1
    // a record at the run's last step
    known_count("last step", ev(10, 0, 5, 0), 0, 10, cnt(1, 0, 2, 0));
    known_count("last step, continued", ev(3, 6, 5, 10), 12, 13, cnt(4, 2, 3, 1));      // 15 18 21 24 | 18 24 | 15 20 25 | 20
    known_count("the issue's run", ev(3, 6, 5, 10), 0, 25, cnt(8, 4, 5, 2));
    // none in a run shorter than the interval
    known_count("shorter than the interval", ev(10, 10, 10, 10), 0, 9, cnt(0, 0, 0, 0));
    known_count("shorter, straddling nothing", ev(10, 0, 0, 7), 21, 6, cnt(0, 0, 0, 0));
    // a record step equal to `first` is the caller's
    known_count("first is a record step", ev(10, 5, 0, 0), 10, 9, cnt(0, 1, 0, 0));
    known_count("first is a record step, run reaches the next", ev(10, 5, 0, 0), 10, 10, cnt(1, 2, 0, 0));
    // all channels off; an empty run
    known_count("all off", ev(0, 0, 0, 0), 0, 1000, cnt(0, 0, 0, 0));
    known_count("empty run", ev(1, 1, 1, 1), 7, 0, cnt(0, 0, 0, 0));
    CHECK(!rec_any(ev(0, 0, 0, 0)) && rec_any(ev(0, 0, 0, 1)), "rec_any");
    // intervals 1 and 2^31 − 1
    known_count("every step", ev(1, 0, 1, 0), 100, 25, cnt(25, 0, 25, 0));
    known_count("2^31 - 1, not reached", ev(BIG, 0, 0, 0), 0, (int64_t)BIG - 1, cnt(0, 0, 0, 0));
    known_count("2^31 - 1, reached at the last step", ev(BIG, 1, 0, 0), (int64_t)BIG - 3, 3, cnt(1, 3, 0, 0));
    known_count("2^31 - 1, twice", ev(BIG, 0, 0, BIG), 0, 2 * (int64_t)BIG, cnt(2, 0, 0, 2));
    known_count("at the largest step numbers", ev(1, 0, 0, BIG), INT64_MAX - 5, 5, cnt(5, 0, 0, 1));      // (2^63 − 2 = (2^31 − 1)·(2^32 + 2))
    // the next record step and its mask
    known_next("all off", ev(0, 0, 0, 0), 0, REC_NEVER, 0);
    known_next("step 0 fires everything that is on", ev(3, 0, 5, 10), 0, 0, 1 | 4 | 8);
    known_next("from 1", ev(3, 6, 5, 10), 1, 3, 1);
    known_next("from 4", ev(3, 6, 5, 10), 4, 5, 4);
    known_next("from 6: KE and PE together", ev(3, 6, 5, 10), 6, 6, 1 | 2);
    known_next("from 28", ev(3, 6, 5, 10), 28, 30, 1 | 2 | 4 | 8);
    known_next("2^31 - 1", ev(0, BIG, 0, 0), 1, BIG, 2);
    known_next("every step", ev(0, 0, 1, 0), 12345, 12345, 4);
    known_next("beyond the largest step number", ev(0, 0, 0, BIG), INT64_MAX, REC_NEVER, 0);      // (2^63 − 2 is the last multiple of 2^31 − 1)
    known_next("the last multiple of 2^31 - 1", ev(0, 0, 0, BIG), INT64_MAX - 2, INT64_MAX - 1, 8);
    // capacity: used + new <= capacity, only for the channels that are on
    ++n_known; CHECK(rec_fits(ev(3, 0, 0, 0), 0, 9, cnt(0, 0, 0, 0), cnt(3, 0, 0, 0)), "three records fit three slots");
    ++n_known; CHECK(!rec_fits(ev(3, 0, 0, 0), 0, 9, cnt(0, 0, 0, 0), cnt(2, 0, 0, 0)), "three records do not fit two slots");
    ++n_known; CHECK(!rec_fits(ev(3, 0, 0, 0), 0, 9, cnt(1, 0, 0, 0), cnt(3, 0, 0, 0)), "three more do not fit behind one");
    ++n_known; CHECK(rec_fits(ev(3, 0, 0, 0), 0, 2, cnt(3, 0, 0, 0), cnt(3, 0, 0, 0)), "a full channel that does not fire fits");
    ++n_known; CHECK(rec_fits(ev(0, 0, 0, 0), 0, 100, cnt(0, 0, 0, 0), cnt(0, 0, 0, 0)), "all off fits nothing into nothing");
    ++n_known; CHECK(!rec_fits(ev(1, 1, 1, 7), 0, 7, cnt(0, 0, 0, 4), cnt(7, 7, 7, 4)), "the last channel is full");
}

static int64_t n_swept = 0;
static void sweep() {
    const int64_t firsts[] = {0, 1, 2, 5, 9, 10, 11, 29, 30, 99, 100, 2147483646};
    const int64_t lengths[] = {0, 1, 2, 3, 9, 10, 11, 25, 60, 61};
    const int32_t iv[] = {0, 1, 2, 3, 5, 10, 60, 2147483647};
    const int64_t caps[] = {0, 1, 2, 7, 100};
    const int n_iv = (int)(sizeof iv / sizeof iv[0]);
    for (int64_t first : firsts) for (int64_t n : lengths)
        for (int a = 0; a < n_iv; ++a) for (int b = 0; b < n_iv; ++b) for (int c = 0; c < n_iv; c += 2) for (int d = 1; d < n_iv; d += 3) {
            const RecEvery e = ev(iv[a], iv[b], iv[c], iv[d]);
            // brute force over the steps of the run
            RecCount want{}; int64_t first_fire = REC_NEVER;
            for (int64_t s = first + 1; s <= first + n; ++s) {
                int m = 0;
                for (int ch = 0; ch < REC_CHANNELS; ++ch) if (e.every[ch] > 0 && s % e.every[ch] == 0) { ++want.n[ch]; m |= 1 << ch; }
                CHECK(rec_mask(e, s) == m, "mask at %lld", (long long)s);
                if (m && first_fire == REC_NEVER) first_fire = s;
            }
            const RecCount got = rec_count(e, first, n);
            for (int ch = 0; ch < REC_CHANNELS; ++ch) CHECK(got.n[ch] == want.n[ch], "first %lld n %lld every %d: %lld vs %lld", (long long)first, (long long)n, e.every[ch], (long long)got.n[ch], (long long)want.n[ch]);
            const int64_t next = rec_next_step(e, first + 1);
            if (first_fire != REC_NEVER) CHECK(next == first_fire, "first %lld n %lld: next %lld vs %lld", (long long)first, (long long)n, (long long)next, (long long)first_fire);
            else CHECK(next > first + n, "first %lld n %lld: next %lld lies inside a run that records nothing", (long long)first, (long long)n, (long long)next);
            // walking the run by rec_next_step visits exactly the record steps
            RecCount walked{};
            for (int64_t s = rec_next_step(e, first + 1); s <= first + n; s = rec_next_step(e, s + 1)) {
                const int m = rec_mask(e, s);
                CHECK(m != 0, "walk stops at %lld, where nothing fires", (long long)s);
                for (int ch = 0; ch < REC_CHANNELS; ++ch) walked.n[ch] += (m >> ch) & 1;
            }
            for (int ch = 0; ch < REC_CHANNELS; ++ch) CHECK(walked.n[ch] == want.n[ch], "walk: channel %d", ch);
            for (int64_t used : caps) for (int64_t cap : caps) {
                if (used > cap) continue;
                bool fits = true;
                for (int ch = 0; ch < REC_CHANNELS; ++ch) if (e.every[ch] > 0 && used + want.n[ch] > cap) fits = false;
                CHECK(rec_fits(e, first, n, cnt(used, used, used, used), cnt(cap, cap, cap, cap)) == fits, "fits: first %lld n %lld used %lld cap %lld", (long long)first, (long long)n, (long long)used, (long long)cap);
                ++n_swept;
            }
        }
}

int main() {
    known_answers();
    sweep();
    std::printf("known answers: %d\nsweep: %lld cases\n", n_known, (long long)n_swept);
    if (failures) { std::printf("record_plan_check: %d FAILED\n", failures); return 1; }
    std::printf("record_plan_check: all passed\n");
    return 0;
}
