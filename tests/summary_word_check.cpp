// summary_word_check.cpp -- the summary word of a 256-voxel segment (semantic_slam_amd/csrc/host_derive.h: encoding and
// word_after_update, the function the one-frame kernel runs on the device) without a device: a stand-alone program
// (tests/test_summary_word.py builds and runs it).  Every expectation below is stated from the rule, not computed with the
// functions under test:
//   bit 0 = every TSDF value is 1, bit 1 = every weight is finite and >= 0, bit 2 = every weight is (float)c, c in bits 8..31;
//   an untouched segment keeps its word; an update that leaves a value != 1 clears bit 0 and nothing else; a run goes on, one
//   higher, only where all 256 voxels were updated and the next count is below 2^24; where it ends, bit 2 and the count go.
// Prints one line per failed case and exits with their number (0 = all good), then "checked N cases".
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "host_derive.h"

using namespace tsdf_host;

static int failures = 0;

static void expect(bool ok, const char *what, uint32_t a, uint32_t b, uint32_t c)
{
    if (ok) return;
    ++failures;
    std::printf("FAILED %s: %08x %08x %08x\n", what, a, b, c);
}

int main()
{
    long cases = 0;
    const uint32_t counts[] = {0u, 1u, (1u << 24) - 2u, (1u << 24) - 1u};

    // ---- the encoding ----
    expect(kSummaryOnes == 1u && kSummarySane == 2u && kSummaryRun == 4u && kRunCountShift == 8, "bit assignment", kSummaryOnes, kSummarySane, kSummaryRun);
    expect(kMaxRunCount == 16777215u, "largest count", kMaxRunCount, 0, 0);
    expect(kSummaryFresh == 7u, "the word of a fresh volume: all three bits, count 0", kSummaryFresh, 0, 0);
    for (uint32_t low = 0; low < 4; ++low) {
        for (uint32_t c : counts) {
            const uint32_t w = word_with_run(low, c);
            ++cases;
            expect(w == (low | 4u | (c << 8)), "word_with_run", low, c, w);
            expect(word_has_run(w) && word_run_count(w) == c, "decode", low, c, w);
            expect((w & 3u) == low, "bits 0 and 1 kept", low, c, w);
            expect(word_without_run(w) == low, "word_without_run", low, c, w);
            expect(!word_has_run(low) && word_run_count(low) == 0u, "no run, no count", low, c, w);
            // the count is the weight: (float)c is exact and has c's value back
            const float f = (float)c;
            expect((uint32_t)f == c && (double)f == (double)c, "count exact in fp32", c, 0, 0);
        }
        // garbage above bit 1 does not pass through the encoder
        expect(word_with_run(low | 0xfffffff8u, 5u) == (low | 4u | (5u << 8)), "word_with_run masks its low argument", low, 0, 0);
    }
    // -0.0f is not the count 0: the rule compares bit patterns
    {
        const float z = 0.0f, nz = -0.0f;
        uint32_t bz, bnz;
        std::memcpy(&bz, &z, 4);
        std::memcpy(&bnz, &nz, 4);
        expect(bz == 0u && bnz == 0x80000000u && bz != bnz, "-0.0f differs from (float)0 in bits", bz, bnz, 0);
    }

    // ---- the transition: {bit 0} x {bit 1} x {bit 2} x counts x {untouched, partly, fully updated} x {value left 1, not} ----
    for (uint32_t bits = 0; bits < 8; ++bits) {
        for (uint32_t c : counts) {
            if (!(bits & 4u) && c != 0u) continue;                  // the count is zero whenever bit 2 is clear
            const uint32_t old = bits | (c << 8);
            for (int how = 0; how < 3; ++how) {                     // 0 untouched, 1 partly, 2 fully updated
                for (int not_one = 0; not_one < 2; ++not_one) {
                    const bool touched = how != 0, all = how == 2;
                    // a segment nothing was updated in cannot have had a value leave 1, and cannot be fully updated; the function
                    // must still ignore both inputs then
                    const uint32_t got = word_after_update(old, touched, all, not_one != 0);
                    ++cases;
                    uint32_t want;
                    if (!touched) {
                        want = old;
                    } else {
                        uint32_t b0 = bits & 1u, b1 = bits & 2u, b2 = bits & 4u, cnt = c;
                        if (not_one) b0 = 0u;
                        if (b2) {
                            if (all && c + 1u < (1u << 24)) cnt = c + 1u;
                            else { b2 = 0u; cnt = 0u; }
                        }
                        want = b0 | b1 | b2 | (cnt << 8);
                    }
                    expect(got == want, "word_after_update", old, (uint32_t)(how * 2 + not_one), got);
                    // invariants, whatever the case: bit 1 never changes; bit 0 is never set; a run is never started; no
                    // count without a run; a count never passes 2^24 - 1
                    expect((got & 2u) == (old & 2u), "bit 1 changed", old, got, 0);
                    expect(!(got & 1u) || (old & 1u), "bit 0 set by an update", old, got, 0);
                    expect(!(got & 4u) || (old & 4u), "run started by an update", old, got, 0);
                    expect((got & 4u) || (got >> 8) == 0u, "count without a run", old, got, 0);
                    expect((got & 0xf8u) == 0u, "bits 3..7 used", old, got, 0);
                    if (!touched) expect(word_after_update(old, false, true, true) == old, "untouched ignores the other inputs", old, got, 0);
                }
            }
        }
    }
    // the limit, spelled out: 2^24 - 2 -> 2^24 - 1 goes on; 2^24 - 1 -> the run ends (the weights become 2^24, then stay: w + 1 == w)
    expect(word_after_update(word_with_run(3u, (1u << 24) - 2u), true, true, false) == word_with_run(3u, (1u << 24) - 1u), "last count", 0, 0, 0);
    expect(word_after_update(word_with_run(3u, (1u << 24) - 1u), true, true, false) == 3u, "count limit ends the run", 0, 0, 0);
    // a chain from a fresh word: n whole updates count to n
    {
        uint32_t w = kSummaryFresh;
        for (uint32_t n = 1; n <= 1000; ++n) {
            w = word_after_update(w, true, true, false);
            if (w != word_with_run(3u, n)) { expect(false, "chain of whole updates", n, w, 0); break; }
        }
        ++cases;
        w = word_after_update(w, true, true, true);             // a band update: bit 0 goes, the run goes on
        expect(w == word_with_run(2u, 1001u), "band update keeps the run", w, 0, 0);
        w = word_after_update(w, true, false, false);           // a partial update ends it
        expect(w == 2u, "partial update ends the run", w, 0, 0);
        w = word_after_update(w, true, true, false);            // and nothing starts it again
        expect(w == 2u, "no run is started", w, 0, 0);
    }
    std::printf("checked %ld cases\n", cases);
    return failures > 255 ? 255 : failures;
}
