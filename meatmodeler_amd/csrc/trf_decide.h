// The host's decisions of the trust-region solve, written once: accept / reject / try again / terminate as SciPy's
// trf_no_bounds takes them (scipy/optimize/_lsq/trf.py:401-560), plus this project's rule for raising the damping when the
// reduced camera system is not positive definite.  Plain C++17, no HIP: both drivers of trf.hip (trf_run behind mm_ba_trf /
// _dist / _fixed, and the lock-step batch) ask this machine what to enqueue next, and tests/trf_decide_replay.cpp compiles
// it alone to hold it against its Python statement (bundleAdjuster._TrfDecide), call by call.
//
// A driver's iteration:   begin() -> BODY | FINAL
//   BODY:   enqueue the body and the first trial step, read the board, on_solve(...)
//             ABANDONED / RETRY: enqueue the reduced solve again (driver policy / with `reg`), on_solve again
//             INDEFINITE: give up;  DONE: gtol stop, the trial is dropped;  USABLE: on_trial(...) with the same board
//   on_trial(...) -> TRIAL: enqueue another trial step with the new Delta, on_trial again
//                    BODY | FINAL: the iteration is closed (`accepted` says how), as begin() would answer
//   FINAL:  enqueue the gradient pass alone, on_final(|g|_inf) -> DONE
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/meatmodeler.h"

namespace mm_trf {

// SciPy's update_tr_radius / check_termination (scipy/optimize/_lsq/common.py:222-245, 705-717)
inline void update_tr_radius(double &Delta, double actual, double predicted, double step_norm, bool bound_hit, double &ratio) {
    if (predicted > 0)
        ratio = actual / predicted;
    else if (predicted == 0 && actual == 0)
        ratio = 1;
    else
        ratio = 0;
    if (ratio < 0.25)
        Delta = 0.25 * step_norm;
    else if (ratio > 0.75 && bound_hit)
        Delta *= 2.0;
}
constexpr int NO_TERMINATION = -100;  // (None)
inline int check_termination(double dF, double F, double dx_norm, double x_norm, double ratio, double ftol, double xtol) {
    const bool ftol_ok = dF < ftol * F && ratio > 0.25;
    const bool xtol_ok = dx_norm < xtol * (xtol + x_norm);
    if (ftol_ok && xtol_ok) return 4;
    if (ftol_ok) return 2;
    if (xtol_ok) return 3;
    return NO_TERMINATION;
}

enum Outcome : int { BODY = 0, TRIAL = 1, FINAL = 2, DONE = 3, RETRY = 4, USABLE = 5, ABANDONED = 6, INDEFINITE = 7 };

struct TrfDecide {
    double Delta, cost, cost0, x_norm = 0.0, step_norm = NAN, actual = NAN, g_norm = NAN;
    double min_damping, reg = 0.0;      // the floor of the damping as raised so far; the damping a RETRY asks for
    int32_t nfev = 1, njev = 1, iteration = 0, termination = NO_TERMINATION, attempt = 0;
    int64_t max_nfev;
    bool accepted = false;              // how the iteration that on_trial just closed ended
    double ftol, xtol, gtol;
    mm_trf_row *log;                    // optional: one row per line of SciPy's verbose=2 table
    int32_t log_cap, n_log = 0;

    // cost: at the initial point; xx_scaled = |x * scale_inv|^2 there (Delta0, trf.py:428); n unknowns
    TrfDecide(double cost_, double xx_scaled, int64_t n, const mm_trf_params &prm, mm_trf_row *log_ = nullptr, int32_t log_cap_ = 0)
        : Delta(std::sqrt(xx_scaled)), cost(cost_), cost0(cost_), min_damping(prm.min_damping > 0 ? prm.min_damping : 1e-9),
          max_nfev(prm.max_nfev > 0 ? prm.max_nfev : 100 * n), ftol(prm.ftol), xtol(prm.xtol), gtol(prm.gtol), log(log_),
          log_cap(log_cap_) {
        if (Delta == 0) Delta = 1.0;
    }

    Outcome begin() const { return termination != NO_TERMINATION || nfev == max_nfev ? FINAL : BODY; }

    // The board of an iteration's first trial step: info of the factorisation, the damping it ran with, |g|_inf, |x|^2.
    Outcome on_solve(int info, double reg_used, double g_norm_, double xx) {
        if (info < 0) return ABANDONED;      // (nothing noted: the driver may issue the same attempt again)
        if (info > 0) {
            if (reg_used <= min_damping * (1.0 + 1e-12)) min_damping *= 100.0;   // failed AT the floor: the floor was too low
            reg = reg_used * 100.0;
            return ++attempt >= 6 ? INDEFINITE : RETRY;
        }
        attempt = 0;
        g_norm = g_norm_;
        if (g_norm < gtol) termination = 1;   // (checked before the step is used, as trf.py:443 does)
        emit_row();
        if (termination != NO_TERMINATION) return DONE;
        x_norm = std::sqrt(xx);
        actual = -1.0;
        return USABLE;
    }

    // A trial step: predicted reduction, |p| in the scaled variables, the unscaled step norm, twice the cost at the trial point.
    Outcome on_trial(double predicted, double step_h_norm, double step_norm_, double cost2_new) {
        const double cost_new = 0.5 * cost2_new;
        ++nfev;
        if (!std::isfinite(cost_new)) {
            Delta = 0.25 * step_h_norm;
        } else {
            actual = cost - cost_new;
            double Delta_new = Delta, ratio;
            update_tr_radius(Delta_new, actual, predicted, step_h_norm, step_h_norm > 0.95 * Delta, ratio);
            step_norm = step_norm_;
            termination = check_termination(actual, cost, step_norm, x_norm, ratio, ftol, xtol);
            if (termination == NO_TERMINATION) Delta = Delta_new;
        }
        if (termination == NO_TERMINATION && actual <= 0 && nfev < max_nfev) return TRIAL;
        accepted = actual > 0;
        if (accepted) {
            cost = cost_new;
            ++njev;
        } else {
            step_norm = 0;
            actual = 0;
        }
        ++iteration;
        return begin();
    }

    Outcome on_final(double g_norm_) {
        g_norm = g_norm_;
        emit_row();
        return DONE;
    }

    void fill(mm_trf_report &rep) const {
        rep.cost0 = cost0;
        rep.cost = cost;
        rep.optimality = g_norm;
        rep.min_damping = min_damping;
        rep.nfev = nfev;
        rep.njev = njev;
        rep.status = termination == NO_TERMINATION ? 0 : termination;
        rep.iterations = iteration;
        rep.log_rows = n_log;
    }

private:
    void emit_row() {
        if (n_log < log_cap) log[n_log] = mm_trf_row{iteration, nfev, cost, actual, step_norm, g_norm};
        ++n_log;
    }
};

}  // namespace mm_trf
