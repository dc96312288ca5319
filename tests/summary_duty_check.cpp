// summary_duty_check.cpp -- what a weight-writing launch owes the summary words, and which kernel one frame runs
// (semantic_slam_amd/csrc/launch_geometry.h: Keeps, SummaryRecord, one_frame -- the code the library's launch sites run) without
// a device: a stand-alone program (tests/test_summary_duty.py builds and runs it).
//
//   summary_duty_check record    every sequence of up to 6 events over {launch keeps nothing, launch keeps bits 0 and 1, launch
//       keeps runs, fill, rebuild} from each of the record's four states, walked beside a model of the device with two facts:
//       every word is zero; some word may carry a run.  The model applies the action the record returns, then the event: fill and
//       a rebuild write every word and may leave runs; a launch that keeps runs writes words and counts as leaving runs; one that
//       keeps bits 0 and 1 writes words too (what it writes is the kernel's business: to the model they are no longer all zero)
//       and touches no run; one that keeps nothing touches nothing.  Held at every step, stated from the rule and not from the
//       record's code:
//         "known zero" implies every word is zero; "no run possible" implies no word carries one;
//         a launch that keeps nothing starts over zero words; a launch that keeps bits 0 and 1 starts with no run anywhere;
//         no action is returned that the model shows to be unnecessary, and none that does not belong to the launch's kind.
//       Ahead of the sweep the 4 x 5 table of single transitions, spelled out.
//   summary_duty_check choice    one line per case "dim_x dim_y nz variant masked kernel keeps" for frames whose tile tables fit:
//       the pytest holds them to tests/summary_spec.py.  The same cases with tables that do not fit are checked here, from the
//       rule: no bricks -- the scalar kernel for rows of no multiple of 4 voxels and for variant 1, else the flat kernel for rows of
//       no multiple of 256 voxels, else integrate_tile.
// Prints one line per failed case, then "checked N cases", and exits with the number of failures (0 = all good).
#include <cstdio>
#include <cstring>

#include "launch_geometry.h"

using namespace tsdf_host;

static int failures = 0;

static void expect(bool ok, const char *what, long a, long b, long c)
{
    if (ok) return;
    ++failures;
    std::printf("FAILED %s: %ld %ld %ld\n", what, a, b, c);
}

enum Event { LaunchNothing, LaunchBits, LaunchRuns, Fill, Rebuild, kEvents };

struct Model { bool zero, run; };

// One event on the record and on the model; `id` names the case in a failure's line.
static void step(SummaryRecord &rec, Model &m, int ev, long id)
{
    if (ev == Fill) { rec.after_fill(); m.zero = false; m.run = true; }
    else if (ev == Rebuild) { rec.after_rebuild(); m.zero = false; m.run = true; }
    else {
        const Keeps keeps = ev == LaunchNothing ? Keeps::Nothing : ev == LaunchBits ? Keeps::Bits : Keeps::Runs;
        const SummaryAction act = rec.before_launch(keeps);
        if (act == SummaryAction::Zero) {
            expect(ev == LaunchNothing, "words zeroed ahead of a launch that keeps them", id, ev, 0);
            expect(!m.zero, "words zeroed that are zero", id, ev, 0);
            m.zero = true; m.run = false;
        } else if (act == SummaryAction::ForgetRuns) {
            expect(ev == LaunchBits, "runs forgotten ahead of a launch that is not of the bits 0 and 1 kind", id, ev, 0);
            expect(m.run, "runs forgotten where there is none", id, ev, 0);
            m.run = false;
        }
        if (ev == LaunchNothing) expect(m.zero, "a launch that keeps nothing starts over words that are not zero", id, ev, 0);
        if (ev == LaunchBits) { expect(!m.run, "a launch that keeps bits 0 and 1 starts with a run", id, ev, 0); m.zero = false; }
        if (ev == LaunchRuns) { m.zero = false; m.run = true; }
    }
    expect(!rec.known_zero || m.zero, "known zero, but not every word is", id, ev, 0);
    expect(rec.runs_maybe || !m.run, "no run possible, but a word may carry one", id, ev, 0);
}

static long check_record()
{
    long cases = 0;
    // single transitions: the state after, and the action, by event and state before
    for (int s = 0; s < 4; ++s) {
        const bool kz = (s & 1) != 0, rm = (s & 2) != 0;
        for (int ev = 0; ev < kEvents; ++ev) {
            SummaryRecord r;
            r.known_zero = kz; r.runs_maybe = rm;
            SummaryAction act = SummaryAction::None;
            if (ev == Fill) r.after_fill();
            else if (ev == Rebuild) r.after_rebuild();
            else act = r.before_launch(ev == LaunchNothing ? Keeps::Nothing : ev == LaunchBits ? Keeps::Bits : Keeps::Runs);
            ++cases;
            // (words known to be zero are left alone, and so is what the record says of runs)
            const bool want_kz = ev == LaunchNothing, want_rm = ev == LaunchRuns || ev == Fill || ev == Rebuild || (ev == LaunchNothing && kz && rm);
            const SummaryAction want = (ev == LaunchNothing && !kz) ? SummaryAction::Zero
                                     : (ev == LaunchBits && rm) ? SummaryAction::ForgetRuns : SummaryAction::None;
            expect(r.known_zero == want_kz && r.runs_maybe == want_rm, "state after a single event", s, ev, r.known_zero + 2 * r.runs_maybe);
            expect(act == want, "action of a single event", s, ev, (long)act);
        }
    }
    // sequences: digits of k in base 5, first event in the lowest digit
    for (int s = 0; s < 4; ++s) {
        long n_seq = 1;
        for (int len = 1; len <= 6; ++len) {
            n_seq *= kEvents;
            for (long k = 0; k < n_seq; ++k) {
                SummaryRecord rec;
                rec.known_zero = (s & 1) != 0; rec.runs_maybe = (s & 2) != 0;
                // the worst the state admits: not zero unless known to be, a run possible unless excluded
                Model m = {rec.known_zero, rec.runs_maybe};
                long d = k;
                for (int i = 0; i < len; ++i, d /= kEvents) step(rec, m, (int)(d % kEvents), (s * 10 + len) * 100000 + k);
                ++cases;
            }
        }
    }
    return cases;
}

static long check_choice()
{
    long cases = 0;
    const int dims_x[] = {3, 4, 36, 252, 256, 260, 512}, dims_y[] = {1, 5, 250}, depths[] = {0, 1, 749, 750}, variants[] = {0, 1, 3, 7, 8};
    const char *kernel_names[] = {"scalar", "flat", "bricks", "tile"}, *keeps_names[] = {"nothing", "bits", "runs"};
    for (int dx : dims_x) for (int dy : dims_y) for (int nz : depths) {
        tsdf_config c;
        std::memset(&c, 0, sizeof c);
        c.dim_x = dx; c.dim_y = dy; c.dim_z = nz > 0 ? nz : 1; c.z_begin = 0; c.z_end = nz;
        c.im_height = 480; c.im_width = 640; c.voxel_size = 0.01f; c.trunc_margin = 0.05f;
        int q, r, s;
        choose_brick_default(c, q, r, s);
        const SlabGeometry g = slab_geometry(c, 16, false, q, r, s);
        for (int variant : variants) for (int masked = 0; masked < 2; ++masked) {
            const Variant var = decode_variant(variant);
            const OneFrame fit = one_frame(g, var, masked != 0, true), nofit = one_frame(g, var, masked != 0, false);
            std::printf("%d %d %d %d %d %s %s\n", dx, dy, nz, variant, masked, kernel_names[(int)fit.kernel], keeps_names[(int)fit.keeps]);
            ++cases;
            const OneFrameKernel want = (dx % 4 != 0 || variant == 1) ? OneFrameKernel::Scalar
                                      : dx % 256 != 0 ? OneFrameKernel::FlatSingle : OneFrameKernel::Tile;
            const Keeps want_keeps = want == OneFrameKernel::Scalar ? Keeps::Nothing : want == OneFrameKernel::Tile ? Keeps::Runs : Keeps::Bits;
            expect(nofit.kernel == want && nofit.keeps == want_keeps, "tables that do not fit", dx * 1000 + dy, nz, variant * 2 + masked);
            ++cases;
        }
    }
    return cases;
}

int main(int argc, char **argv)
{
    long cases = 0;
    if (argc == 2 && std::strcmp(argv[1], "record") == 0) cases = check_record();
    else if (argc == 2 && std::strcmp(argv[1], "choice") == 0) cases = check_choice();
    else { std::printf("usage: summary_duty_check record|choice\n"); return 2; }
    std::printf("checked %ld cases\n", cases);
    return failures > 255 ? 255 : failures;
}
