// mg_schedule.hpp -- the V(nu, nu) cycle of kind "multigrid" as a schedule: which operation runs on which level in which order, and
// which ONE step of a cycle writes the r.z partials (include/spmv_amd/api.h, steps (1)-(5) of spmv_amd_precond_create_multigrid's
// text). Standard headers only: no HIP, nothing here launches, so tests/abi/mg_schedule_test.cpp walks it on a CPU. The single-vector
// cycle (multigrid.hip) and the batched one (multigrid_multi.hip) are two Ops on this one walk: that is what keeps a batched column's
// bits those of the single-vector cycle.
#ifndef SPMV_AMD_MG_SCHEDULE_HPP
#define SPMV_AMD_MG_SCHEDULE_HPP

namespace spmv_amd {

// Level: anything with `int degree` (Chebyshev steps of the level's smoother; the coarsest level: of its solve) and `coef` (c0, h_1,
// g_1, h_2, g_2, ...). Ops: term0(l) -- u = dinv r ; d = c0 u ; z = d --, step(l, g, h, last) -- one update t = r - A z ; u = dinv t ;
// d = g u + h d ; z = z + d; last: this step also writes the r.z partials --, restrict_residual(l) -- level l + 1's r from level l's
// z and r --, prolong(l) -- level l + 1's z into level l's.
template <class Level, class Ops>
void mg_vcycle(Ops& ops, const Level* levels, int count, int l = 0) {
    const Level& L = levels[l];
    const bool coarsest = l + 1 == count, top = l == 0;
    auto steps = [&](bool report) {
        for (int s = 1; s <= L.degree; ++s) ops.step(l, L.coef[2 * s], L.coef[2 * s - 1], report && s == L.degree);
    };
    ops.term0(l);
    steps(coarsest && top);  // pre-smoothing; the coarsest level: its solve
    if (coarsest) return;
    ops.restrict_residual(l);
    mg_vcycle(ops, levels, count, l + 1);
    ops.prolong(l);
    ops.step(l, L.coef[0], 0.0, top && L.degree == 0);  // post-smoothing from the guess z: term 0 in step form
    steps(top);
}

}  // namespace spmv_amd
#endif
