// Stand-alone host program for tests/test_selinv_plan.py: the selected
// inverse's planner (vlgba_debug_selinv_plan, csrc/ba_chol_plan.cpp) for tile
// counts 1 .. 40 and 200, with exactly-sized output arrays so that a
// sanitizer build sees any write past them.  Prints "selinv <ntiles> <levels>"
// per count and checks the lists' invariants itself; exit 0 when all hold.
#include "vlgba.h"

#include <cstdio>
#include <vector>

static int check(int nt)
{
    std::vector<int> elim(3 * (size_t)nt), eptr(34), src(2 * (size_t)nt);
    const int nl = vlgba_debug_selinv_plan(nt, elim.data(), eptr.data(), src.data());
    if (nl < 1 || eptr[0] != 0 || eptr[nl] != nt) return 1;
    std::vector<int> rec(nt, -1);
    for (int i = 0; i < nt; i++) {
        const int e = elim[3 * i];
        if (e < 0 || e >= nt || rec[e] >= 0) return 2;
        rec[e] = i;
    }
    for (int i = 0; i < nt; i++) {
        const int p = elim[3 * i + 1], q = elim[3 * i + 2], s = src[2 * i], t = src[2 * i + 1];
        if ((p < 0 || q < 0) != (s < 0)) return 3;
        if (s < 0) continue;
        if (s >= nt || (t != 0 && t != 1)) return 4;
        // the source is p's record with q as its upper neighbour, or q's with p below
        if (t ? (elim[3 * s] != p || elim[3 * s + 2] != q) : (elim[3 * s] != q || elim[3 * s + 1] != p))
            return 5;
    }
    std::printf("selinv %d %d\n", nt, nl);
    return 0;
}

int main()
{
    for (int nt = 1; nt <= 40; nt++)
        if (int rc = check(nt)) return rc;
    if (int rc = check(200)) return rc;
    int one[3], ep[34], sr[2];
    if (vlgba_debug_selinv_plan(0, one, ep, sr) != -1) return 6;
    if (vlgba_debug_selinv_plan(1, nullptr, ep, sr) != -1) return 7;
    return 0;
}
