// d2d_layout.h -- the scenario-grouped slot layout of libdrone2d_hip.so: which env sits in which state
// slot, which K1 workgroup steps which group of slots.  Pure host code (make_groups, balance_groups)
// plus the one function host and kernels share (xcd_group).  Includes nothing from HIP, so a plain
// C++ compiler builds it (tests/layout_host_main.cpp); included by d2d_kernels.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

// host + device under hipcc, plain inline elsewhere
#if defined(__HIPCC__)
#define D2D_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define D2D_HD inline
#endif

namespace d2dk {

constexpr int EPB = 64;  // K1: envs per workgroup = slots per group

// Workgroup renumbering for the grouped lane map: blocks b and b + 8 share an XCD (and its L2)
// when the grid is dealt round-robin over the 8 XCDs, so consecutive group numbers -- groups whose
// envs share cache lines -- go to blocks on one XCD.  Placement only affects speed.
// XCD x = b % 8 holds per + (x < rem) blocks; its k-th block (k = b / 8) takes group number
// (groups of XCDs before x) + k, a bijection on [0, nb).
D2D_HD int xcd_group(int b, int nb) {
    const int per = nb / 8, rem = nb % 8, x = b % 8, k = b / 8;
    return (x < rem) ? x * (per + 1) + k : rem * (per + 1) + (x - rem) * per + k;
}

// Scenario-grouped slot layout for a static env -> scenario map with several scenarios: each K1
// workgroup then steps 64 envs of ONE scenario (no per-lane scenario divergence in the Brent
// search, one scenario + probe table staged in LDS) whose state is contiguous.  The envs, sorted
// by (scenario, id), are cut into ceil(n / 64) groups -- no padding between scenarios, so the grid
// is no larger than the identity layout's (at 65 536 envs: 1 024 workgroups = one resident round)
// and at most n_scn - 1 groups straddle scenarios: wg_scn = -(s + 2) for a group of scenarios s and
// s + 1 (K1 stages both scenarios in LDS; their probe tables are read through L1/L2), -1 for a group
// of three or more (everything through L1/L2).  Groups are then
// ordered by their first env id, so groups whose envs interleave (e.g. scenario = id mod 7) get
// consecutive numbers (xcd_group places consecutive numbers on one XCD).
// lanes: slot -> env (-1: padding), ws: wg_scn per group.
inline void make_groups(int n, const int32_t* env_scn, std::vector<int32_t>& lanes, std::vector<int32_t>& ws) {
    std::vector<int32_t> order((size_t)n);
    for (int i = 0; i < n; ++i) order[(size_t)i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return env_scn[x] < env_scn[y]; });
    const size_t ng = ((size_t)n + EPB - 1) / EPB;
    std::vector<size_t> gi(ng);
    for (size_t g = 0; g < ng; ++g) gi[g] = g;
    std::sort(gi.begin(), gi.end(), [&](size_t x, size_t y) { return order[x * EPB] < order[y * EPB]; });
    lanes.assign(ng * EPB, -1);
    ws.assign(ng, 0);
    for (size_t g = 0; g < ng; ++g) {
        const size_t o = gi[g] * EPB;
        const int32_t lo = env_scn[order[o]];
        int32_t hi = lo;
        for (size_t l = 0; l < EPB && o + l < (size_t)n; ++l) {
            lanes[g * EPB + l] = order[o + l];
            hi = std::max(hi, env_scn[order[o + l]]);
        }
        // pure: the scenario; straddling exactly two consecutive scenarios: -(lo + 2); more: -1
        ws[g] = hi == lo ? lo : (hi == lo + 1 ? -(lo + 2) : -1);
    }
}

constexpr double STRADDLE_W = 1.25;  // balance_groups: a straddling group's cost over its heavier scenario's
// Co-residency balance (mixed batches).  When every workgroup of K1 is resident at once (ng <= 4 x
// CUs), the dispatcher fills the CUs round by round in one fixed CU order, so blocks b, b + n_cu,
// b + 2 n_cu, ... share a CU (measured on MI355X: blocks congruent mod 256 share a CU, in every step
// of a replayed graph, tools/cu_map.py).  A step lasts as long as its slowest workgroup, and a heavy
// scenario's workgroup slows down when its CU also runs other heavy ones, so the groups of each XCD's
// chunk (xcd_group keeps a chunk of consecutive group numbers on one XCD) are dealt over the chunk's
// CUs by cost, heaviest first onto the least-loaded CU (straddling groups count 1.25 x their heavier
// scenario; a scenario beyond the cost table counts as the dearest).  Renumbers the groups (lanes / ws)
// in place; the arithmetic is unchanged.
inline void balance_groups(int n_cu, const double* cost, int n_cost, std::vector<int32_t>& lanes,
                           std::vector<int32_t>& ws) {
    const int ng = (int)ws.size();
    if (n_cu <= 0 || n_cu % 8 != 0 || ng > 4 * n_cu || ng < 2) return;
    double cmax = 0.0;
    for (int k = 0; k < n_cost; ++k) cmax = std::max(cmax, cost[k]);
    auto c = [&](int sc) { return (sc >= 0 && sc < n_cost) ? cost[sc] : cmax; };
    auto gcost = [&](int g) {
        const int w = ws[(size_t)g];
        return w >= 0 ? c(w) : (w <= -2 ? STRADDLE_W * std::max(c(-w - 2), c(-w - 1)) : 1.5 * cmax);
    };
    std::vector<int32_t> block_of((size_t)ng);  // group number -> the block that runs it
    for (int b = 0; b < ng; ++b) block_of[(size_t)xcd_group(b, ng)] = b;
    std::vector<int32_t> newnum((size_t)ng, -1);
    const int per = ng / 8, rem = ng % 8;
    for (int x = 0, first = 0; x < 8; ++x) {
        const int cnt = per + (x < rem ? 1 : 0);
        // the chunk's positions grouped by CU, each CU's positions in dispatch order
        std::vector<std::pair<int, int>> pos;  // (cu, position)
        for (int p = first; p < first + cnt; ++p) pos.emplace_back(block_of[(size_t)p] % n_cu, p);
        std::stable_sort(pos.begin(), pos.end(), [&](const std::pair<int, int>& u, const std::pair<int, int>& v) {
            return u.first != v.first ? u.first < v.first : block_of[(size_t)u.second] < block_of[(size_t)v.second];
        });
        std::vector<int> cus;
        std::vector<std::vector<int>> free_pos;
        for (const auto& q : pos) {
            if (cus.empty() || cus.back() != q.first) {
                cus.push_back(q.first);
                free_pos.emplace_back();
            }
            free_pos.back().push_back(q.second);
        }
        std::vector<double> load(cus.size(), 0.0);
        std::vector<size_t> used(cus.size(), 0);
        std::vector<int> gs;
        for (int g = first; g < first + cnt; ++g) gs.push_back(g);
        std::stable_sort(gs.begin(), gs.end(), [&](int u, int v) { return gcost(u) > gcost(v); });
        for (int g : gs) {
            size_t best = cus.size();
            for (size_t k = 0; k < cus.size(); ++k)
                if (used[k] < free_pos[k].size() && (best == cus.size() || load[k] < load[best])) best = k;
            newnum[(size_t)g] = free_pos[best][used[best]++];
            load[best] += gcost(g);
        }
        first += cnt;
    }
    std::vector<int32_t> l2(lanes.size(), -1), w2((size_t)ng, 0);
    for (int g = 0; g < ng; ++g) {
        const size_t d = (size_t)newnum[(size_t)g];
        w2[d] = ws[(size_t)g];
        for (int l = 0; l < EPB; ++l) l2[d * EPB + (size_t)l] = lanes[(size_t)g * EPB + (size_t)l];
    }
    lanes.swap(l2);
    ws.swap(w2);
}

}  // namespace d2dk
