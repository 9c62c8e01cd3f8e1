// Replays a list of boards through TrfDecide (meatmodeler_amd/csrc/trf_decide.h) the way a driver would and writes out the
// outcome and the full state after every call: tests/test_trf_decisions_cpu.py holds the trace against the Python
// statement of the same machine.  Built by the test itself (g++ -std=c++17 -O1 -ffp-contract=off), linked into nothing else.
#include "trf_decide.h"

using namespace mm_trf;

namespace {
constexpr int N_BOARD = 8;       // info, reg_used, |g|_inf, |x|^2, predicted, step_h_norm, step_norm, 2 * cost_new
constexpr int N_RECORD = 18;     // outcome + the 17 fields below

void record(double *r, int outcome, const TrfDecide &d) {
    const double v[N_RECORD] = {(double)outcome, d.Delta, d.cost, d.cost0, d.x_norm, d.step_norm, d.actual, d.g_norm, d.min_damping,
                                d.reg, (double)d.nfev, (double)d.njev, (double)d.iteration, (double)d.termination, (double)d.attempt,
                                (double)d.max_nfev, d.accepted ? 1.0 : 0.0, (double)d.n_log};
    for (int i = 0; i < N_RECORD; ++i) r[i] = v[i];
}
}  // namespace

// boards [n_boards, 8] in the order they arrive; records [record_cap, 18], one per call of the machine (begin included).
// Returns the number of calls made (the replay ends with DONE, INDEFINITE, or the last board), or -1 if record_cap is too small.
extern "C" int trf_decide_replay(const mm_trf_params *prm, double cost0, double xx_scaled, int64_t n, const double *boards, int n_boards,
                                 double *records, int record_cap, mm_trf_row *log, int log_cap, mm_trf_report *rep) {
    TrfDecide d(cost0, xx_scaled, n, *prm, log, log_cap);
    int calls = 0;
    auto note = [&](Outcome o) {
        if (calls < record_cap) record(records + (size_t)calls * N_RECORD, o, d);
        ++calls;
        return o;
    };
    Outcome state = note(d.begin());
    for (int b = 0; b < n_boards && state != DONE && state != INDEFINITE; ++b) {
        const double *bd = boards + (size_t)b * N_BOARD;
        if (state == FINAL) {
            state = note(d.on_final(bd[2]));
            continue;
        }
        if (state != TRIAL) {      // BODY, or the reduced solve again after RETRY / ABANDONED
            state = note(d.on_solve((int)bd[0], bd[1], bd[2], bd[3]));
            if (state != USABLE) continue;
        }
        state = note(d.on_trial(bd[4], bd[5], bd[6], bd[7]));
    }
    d.fill(*rep);
    return calls <= record_cap ? calls : -1;
}
