// Stand-alone host program over csrc/d2d_layout.h (built with the address and undefined-behaviour
// sanitizers by tests/test_abi.py::test_layout_host_code_sanitized): the maps of
// test_group_layout_properties, the (n, n_cu) pairs of test_balanced_group_layout, and the edges.
// Exit status 0: every property held and the sanitizers saw nothing.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>

#include "d2d_layout.h"

using d2dk::EPB;
using Map = std::vector<int32_t>;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, g_case); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)
static char g_case[128] = "";

// the properties of make_groups (tests/test_abi.py test_group_layout_properties)
static void check_groups(const Map& es, int k, const Map& lanes, const Map& ws) {
    const int n = (int)es.size(), ng = (n + EPB - 1) / EPB;
    CHECK((int)ws.size() == ng && (int)lanes.size() == ng * EPB);
    Map env_slot((size_t)n, -1);  // env <-> slot is a bijection
    int pad = 0;
    for (int s = 0; s < ng * EPB; ++s) {
        const int e = lanes[(size_t)s];
        if (e < 0) {
            CHECK(e == -1);
            ++pad;
            continue;
        }
        CHECK(e < n && env_slot[(size_t)e] == -1);
        env_slot[(size_t)e] = s;
    }
    CHECK(pad == ng * EPB - n);
    int straddle = 0;
    for (int g = 0; g < ng; ++g) {
        std::set<int> scn;
        int prev_s = -1, prev_e = -1;
        for (int l = 0; l < EPB; ++l) {
            const int e = lanes[(size_t)(g * EPB + l)];
            if (e < 0) continue;
            const int s = es[(size_t)e];
            CHECK(s > prev_s || (s == prev_s && e > prev_e));  // (scenario, id) order inside a group
            prev_s = s, prev_e = e;
            scn.insert(s);
        }
        const int w = ws[(size_t)g];
        CHECK(!scn.empty() && lanes[(size_t)g * EPB] >= 0);
        if (w >= 0) {
            CHECK(w < k && scn.size() == 1 && *scn.begin() == w);
        } else if (w <= -2) {
            ++straddle;
            CHECK(scn.size() == 2 && *scn.begin() == -w - 2 && *scn.rbegin() == -w - 1);
        } else {
            ++straddle;
            CHECK(w == -1 && (scn.size() > 2 || (scn.size() == 2 && *scn.rbegin() > *scn.begin() + 1)));
        }
    }
    CHECK(straddle <= k - 1);
}

// balancing only permutes groups (ws with its 64 lanes), and not at all where it must not
static void check_balanced(const Map& lanes0, const Map& ws0, const Map& lanes, const Map& ws, bool identity) {
    CHECK(lanes.size() == lanes0.size() && ws.size() == ws0.size());
    if (identity) {
        CHECK(lanes == lanes0 && ws == ws0);
        return;
    }
    std::map<Map, int32_t> rows;  // a group's lanes -> its wg_scn (first envs differ: no two rows are equal)
    for (size_t g = 0; g < ws0.size(); ++g)
        rows[Map(lanes0.begin() + (long)(g * EPB), lanes0.begin() + (long)((g + 1) * EPB))] = ws0[g];
    CHECK(rows.size() == ws0.size());
    for (size_t g = 0; g < ws.size(); ++g) {
        auto it = rows.find(Map(lanes.begin() + (long)(g * EPB), lanes.begin() + (long)((g + 1) * EPB)));
        CHECK(it != rows.end() && it->second == ws[g]);
        rows.erase(it);
    }
    CHECK(rows.empty());
}

static void run(const char* name, const Map& es, int k, const std::vector<double>& cost, const std::vector<int>& n_cus) {
    const int n = (int)es.size(), ng = (n + EPB - 1) / EPB;
    Map lanes0, ws0;
    d2dk::make_groups(n, es.data(), lanes0, ws0);
    std::snprintf(g_case, sizeof g_case, "%s n=%d", name, n);
    check_groups(es, k, lanes0, ws0);
    for (size_t g = 1; g < ws0.size(); ++g) CHECK(lanes0[g * EPB] > lanes0[(g - 1) * EPB]);  // numbered by first env id
    for (int n_cu : n_cus) {
        std::snprintf(g_case, sizeof g_case, "%s n=%d n_cu=%d n_cost=%d", name, n, n_cu, (int)cost.size());
        Map lanes = lanes0, ws = ws0;
        d2dk::balance_groups(n_cu, cost.data(), (int)cost.size(), lanes, ws);
        check_balanced(lanes0, ws0, lanes, ws, n_cu <= 0 || n_cu % 8 != 0 || ng > 4 * n_cu || ng < 2);
        check_groups(es, k, lanes, ws);
    }
}

int main() {
    // xcd_group: a bijection on [0, nb) that keeps each XCD's blocks on consecutive numbers
    for (int nb : {1, 2, 7, 8, 9, 13, 16, 63, 64, 65, 1023, 1024, 1025}) {
        std::snprintf(g_case, sizeof g_case, "xcd_group nb=%d", nb);
        std::vector<int> seen((size_t)nb, 0);
        for (int b = 0; b < nb; ++b) {
            const int g = d2dk::xcd_group(b, nb);
            CHECK(g >= 0 && g < nb && !seen[(size_t)g]++);
            if (b >= 8) CHECK(g == d2dk::xcd_group(b - 8, nb) + 1);
        }
    }
    // scenario step costs of the seven named scenarios (config.py SCENARIO_STEP_COST, in the tests' order)
    const std::vector<double> cost7 = {31.2, 31.3, 43.8, 32.4, 45.1, 41.5, 32.4};
    const std::vector<int> cus = {0, 8, 100, 256};
    auto mod = [](int n, int k) {
        Map es((size_t)n);
        for (int i = 0; i < n; ++i) es[(size_t)i] = i % k;
        return es;
    };
    // the four maps of test_group_layout_properties
    run("mod7", mod(65536, 7), 7, cost7, cus);
    {
        // ragged: uneven shares, scenario 5 with three envs, scenario 6 with none
        Map es(1001);
        uint32_t x = 11;
        for (auto& v : es) {
            x = x * 1664525u + 1013904223u;
            const uint32_t u = (x >> 8) % 100;
            v = u < 30 ? 0 : u < 55 ? 1 : u < 75 ? 2 : u < 90 ? 3 : 4;
        }
        es[5] = es[500] = es[1000] = 5;
        run("ragged", es, 7, cost7, cus);
    }
    run("single", Map(300, 2), 3, {1.0, 2.0, 3.0}, cus);
    run("tiny", Map{3, 0, 3, 1, 0}, 4, {1.0, 1.0, 1.0, 1.0}, cus);
    // the (n, n_cu) pairs of test_balanced_group_layout (n_cu = 0, a non-multiple of 8, ng > 4 n_cu = 32 included)
    for (int n : {65536, 32768, 65536 + 37, 1001}) run("balanced", mod(n, 7), 7, cost7, cus);
    // edges: one group or barely two; a scenario with no envs; a cost table shorter than the scenario
    // count (the missing scenarios count as the dearest) and an empty one
    for (int n : {1, 63, 64, 65}) {
        run("edge", mod(n, 3), 3, {1.0, 2.0, 3.0}, cus);
        run("edge-empty-scenario", mod(n, 2), 4, {1.0, 2.0, 3.0, 4.0}, cus);
    }
    run("short-cost", mod(1001, 7), 7, {31.2, 31.3, 43.8}, cus);
    run("short-cost", mod(4096, 7), 7, {5.0}, cus);
    run("no-cost", mod(4096, 7), 7, {}, cus);
    {
        Map es = mod(4096, 7);  // scenario 3 has no envs: groups straddle 2 and 4 (three-or-more marking)
        for (auto& v : es)
            if (v == 3) v = 4;
        run("empty-scenario", es, 7, cost7, cus);
    }
    std::puts("layout host code: ok");
    return 0;
}
