// What the host driver of the device remesher (nw_remesh_dev.hip) decides, without HIP: how much room an attempt gets and how often it
// doubles, when a pass has run dry with reports that may not be in yet, when a split sweep is left to the next iteration, when the
// iterations stop, and the Morton cube of the input.  Plain C++14 over the standard library: nw_remesh_dev.hip includes it,
// tests/test_remesh_plan_cpu.py compiles it for the CPU with g++ and holds it against tests/remesh_device_ref.py.
#pragma once
#include <cstdint>
#include <cstddef>
#include <cstdlib>
#include <algorithm>
#include <limits>

namespace rm_plan {

const int R_MAX[3] = {24, 32, 24};   // rounds of a split / collapse / flip pass at most
enum { ROUNDS_CAP = 4096 };          // rounds of one call (numbered through; a call that needs more stops early)
enum { RUN_AHEAD = 2 };              // rounds the host may launch beyond the last report it has waited for
enum { SPLIT_SWEEPS = 4 };           // split passes of one iteration at most (the host code's sweeps: up to 8)
enum { TRIES = 8 };                  // attempts of one call at most, each with twice the room of the one before

// what a round's keys are hashed with: no two rounds of a call share it (a pass has fewer than 64 rounds)
inline unsigned round_seed(unsigned pass_no, int r) { return pass_no * 64u + (unsigned)r; }

// edges longer than `high` are split, shorter than `low` collapsed (Botsch & Kobbelt 2004)
inline double edge_high(double L) { return 4.0 / 3.0 * L; }
inline double edge_low(double L) { return 4.0 / 5.0 * L; }

inline int effective_max_valence(int max_valence) { return max_valence > 0 ? std::min(max_valence, 60) : 16; }

// ---- room -------------------------------------------------------------------------------------------------------------------------------
// Capacities are fixed per attempt: room for the faces the lengths call for (or the input's, if that is more) times `room`; a split
// adds two faces and one vertex; three half-edges a face; a candidate list holds one half-edge of an edge.  (A room below 1 is the tests'
// knob for small inputs.  Nothing here keeps Fcap at nf_in or above: below it, Vcap's difference wraps around.)
enum Fit { FITS = 0, RUNAWAY /* a bad argument */, TOO_LARGE /* out of memory */ };
struct Capacity { size_t Fcap, Vcap, Hcap, list; };
inline Fit capacities(double pieces, int64_t nv_in, int64_t nf_in, double room, Capacity *c)
{
    if (!(pieces < 67108864.0)) return RUNAWAY;                      // (the host code's "runaway": a vertex flung far away)
    const double want = std::max(pieces, (double)nf_in) * room + 8192.0;
    if (want > 5.0e8) return TOO_LARGE;
    c->Fcap = (size_t)want;
    c->Vcap = (size_t)nv_in + (c->Fcap - (size_t)nf_in) / 2 + 1024;
    c->Hcap = 3 * c->Fcap;
    c->list = c->Hcap / 2 + 64;
    return FITS;
}

// the first attempt's room: 1.5, or what NW_REMESH_ROOM says (tests: start too small, so that the retry runs); every later one doubles it
inline double first_room(const char *env) { return env ? std::max(0.05, std::atof(env)) : 1.5; }
inline double next_room(double room) { return room * 2.0; }

// ---- the end of a pass, of the split sweeps, of the iterations --------------------------------------------------------------------------
// Is round r of a pass launched?  reports[j], j < r: the bidders of the pass's round j as the host sees them now, -1 = not in yet (the
// caller has waited for reports[r - RUN_AHEAD]); first: the number of the pass's round 0 within the call.
// A pass ends when a reported round had no bidder -- or so few that the next iteration may as well have them (a tail of a handful of
// candidates that keep losing to each other took as many rounds as all the others).  An empty round may be noticed whenever its report
// happens to be in -- the rounds behind it do nothing either way --, but the "so few" rule decides whether real work is done: it looks at
// the rounds up to the one before last only, whose reports the host has waited for.
inline bool launches_round(const volatile int *reports, int r, unsigned first)
{
    bool dry = false;
    int first_bids = -1;
    for (int j = 0; j < r; ++j) {
        const int b = reports[j];
        if (j == 0 && b >= 0) first_bids = b;
        dry = dry || b == 0 || (j + RUN_AHEAD <= r && b > 0 && first_bids > 0 && b < 8 && b * 500 < first_bids);
    }
    return !dry && first + (unsigned)r < (unsigned)ROUNDS_CAP;
}

// What the splits of a sweep leave too long is the next sweep's; a sweep over a handful of edges -- a scan over all half-edges, a
// compaction and a few rounds for six edges of 4 10^5 -- is left to the next iteration, as the rounds' tails are.
inline bool sweeps_end(int n_list, int first_list) { return n_list < 32 && n_list * 200 < first_list; }

// A pass that changed nothing would be repeated unchanged by every later iteration (with relaxation every vertex moves: the next
// iteration sees another mesh).  before / now: the split, collapse and flip counters at the iteration's start and end.
inline bool iterations_end(int n_relax, const int before[3], const int now[3])
{
    return n_relax == 0 && now[0] == before[0] && now[1] == before[1] && now[2] == before[2];
}

// ---- the Morton cube of the input -------------------------------------------------------------------------------------------------------
// the result's vertices are ordered by the Morton code of their cell in a cube of 1024^3 cells at `lo` with the input's largest extent
struct Cube { double lo[3], per_unit; };
inline Cube morton_cube(const float *vertices, int64_t nv)
{
    const double inf = std::numeric_limits<double>::infinity();
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int64_t v = 0; v < nv; ++v)
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], (double)vertices[3 * v + k]); hi[k] = std::max(hi[k], (double)vertices[3 * v + k]); }
    const double ext = std::max({hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2], 1e-30});
    return Cube{{lo[0], lo[1], lo[2]}, 1024.0 / ext};
}

}  // namespace rm_plan
