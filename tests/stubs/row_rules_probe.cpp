// Test helper (tests/test_row_rules.py): the product's own row rules (armour_amd/csrc/row_rules.h), host side, on one table.
// stdin: a slv::RowRule, a slv::RowLimits, the torque radii [n][T], g [m], all raw.  stdout, raw doubles: g_l [m], g_u [m] (row_bounds),
// outside [m] (outside_slack on those bounds), then the record l1, worst, worst_row, n_violated, n_outside_slack, feasible -- 256 partial
// records filled as thread t of the kernels fills its own (rows t, t + 256, ... ascending) and combined by the kernels' tree, step by step.
#include <cstdio>
#include <vector>

#include "../../armour_amd/csrc/row_rules.h"

int main() {
    slv::RowRule R;
    slv::RowLimits L;
    if (fread(&R, sizeof R, 1, stdin) != 1 || fread(&L, sizeof L, 1, stdin) != 1) return 2;
    if (R.n < 1 || R.n > ARMOUR_MAX_FACTORS || R.T < 1 || R.m < 0 || R.m > (1 << 20) || R.m != R.row0 + R.Q + 4 * R.n) return 2;
    std::vector<double> tr((size_t)R.n * R.T), g((size_t)R.m), out;
    if (fread(tr.data(), sizeof(double), tr.size(), stdin) != tr.size() || fread(g.data(), sizeof(double), g.size(), stdin) != g.size()) return 2;
    std::vector<double> l((size_t)R.m), u((size_t)R.m);
    for (int r = 0; r < R.m; r++) slv::row_bounds(R, L, r, tr.data(), &l[r], &u[r]);
    out.insert(out.end(), l.begin(), l.end());
    out.insert(out.end(), u.begin(), u.end());
    for (int r = 0; r < R.m; r++) out.push_back(slv::outside_slack(R, r, g[r], l[r], u[r]) ? 1.0 : 0.0);
    static slv::ViolShared<1> sh;
    for (int tid = 0; tid < 256; tid++) {
        slv::ViolPartial p;
        for (int r = tid; r < R.m; r += 256) p.take(R, r, g[r], l[r], u[r]);
        p.store(sh, 0, tid);
    }
    for (int s = 128; s > 0; s >>= 1)
        for (int tid = 0; tid < s; tid++) slv::ViolPartial::tree_step(sh, 0, tid, s);
    const ArmourViolation v = slv::ViolPartial::finish(sh, 0);
    const double rec[6] = {v.l1_violation, v.worst, (double)v.worst_row, (double)v.n_violated, (double)v.n_outside_slack, (double)v.feasible};
    out.insert(out.end(), rec, rec + 6);
    if (fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size()) return 1;
    return fflush(stdout) == 0 ? 0 : 1;
}
