// d2d_hip.hip -- C ABI of libdrone2d_hip.so (see include/drone2d.h): the handle, its device buffers,
// and the launches of the kernels in d2d_kernels.h (K1 cooperative step, K2 masked reset, K3 episode
// statistics, K4 reset observation cache fill, K5 fresh curriculum).  The slot layout's host code is
// d2d_layout.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "d2d_kernels.h"

using namespace d2dk;

namespace {
thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int hip_fail(hipError_t e, const char* what) {
    return fail(D2D_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// Owned device memory: freed when the owner goes out of scope or is assigned over.
struct HipFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
template <class T>
using DevBuf = std::unique_ptr<T, HipFree>;
// `count` elements of device memory set to the byte `fill`, the first n_src of them copied from host `src`
template <class T>
hipError_t dev_new(DevBuf<T>& out, size_t count, int fill = 0, const T* src = nullptr, size_t n_src = 0) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, sizeof(T) * count);
    if (e != hipSuccess) return e;
    out.reset(static_cast<T*>(p));
    if (n_src < count) e = hipMemset(p, fill, sizeof(T) * count);
    if (e == hipSuccess && n_src) e = hipMemcpy(p, src, sizeof(T) * n_src, hipMemcpyHostToDevice);
    return e;
}

// Internal arrays of one slot layout.
struct Layout {
    int ns = 0;  // state slots (columns of the [F][ns] arrays): n, or the grouped layout's 64 per group
    DevBuf<double> st;
    DevBuf<int32_t> ist;
    DevBuf<double> acc;
    // auto-reset observation cache (d2d_kernels.h, "Auto-reset observation cache")
    DevBuf<float> rc_obs;    // [RC_SLOTS][ns][27]
    DevBuf<int32_t> rc_rfl;  // [RC_SLOTS][ns]
    DevBuf<int32_t> rc_tag;  // [RC_SLOTS][ns]
    // scenario-grouped slot layout (StepArgs::lane_env); null: slot == env
    DevBuf<int32_t> lane_env;  // [ns] slot -> env (-1: padding)
    DevBuf<int32_t> wg_scn;    // [ns / EPB] scenario of each slot group
    DevBuf<int32_t> env_slot;  // [n] env -> slot
    bool grouped() const { return lane_env != nullptr; }
    int n_groups() const { return grouped() ? ns / EPB : 0; }
};
// The scenario table and what is derived from it.
struct ScnTables {
    int n_scn = 0;              // entries (pool mode: both halves; fresh mode: 2 per env)
    bool rm = false;            // the table's layout: ScnR where K1 reads it from global memory (place)
    DevBuf<unsigned char> scn;  // ABI scenarios + derived fields, ScnF or ScnR
    DevBuf<d2d::BrTab> brt;     // golden-march tables of the scenarios (d2d_brtab_kernel); fresh mode: none
    DevBuf<d2d_scn> abi;        // ABI records of the table (pool and fresh modes: readback)
};
// Fresh curriculum: per scenario slot, the episode it was generated for, and K5's queue.
struct FreshSlots {
    DevBuf<int32_t> scn_tag;  // [2 n] episode key of each slot
    DevBuf<int64_t> gclk;     // [2 n] clock at generation
    DevBuf<int32_t> queue;    // [ring + FR_WORDS] K5's ring of slots to generate + its words
    size_t ring = 0;          // ring size: the power of two >= 2 n
    uint32_t* words() const { return reinterpret_cast<uint32_t*>(queue.get() + ring); }
};
}  // namespace

struct d2d_handle {
    d2d_cfg cfg;
    int n = 0;
    int device = 0;
    int n_cu = 0;  // compute units of the device
    Layout lay;
    ScnTables tab;
    FreshSlots fresh;
    DevBuf<int32_t> env_scn;
    // pool mode: the scenario table has two halves of pool_n entries; resets draw from the half at
    // pool_base (host copy; the kernels read *pool_dev), d2d_refresh_pool fills and switches halves
    int pool_base = 0, pool_n = 0;
    int pool_valid = 0;  // bit h = half h holds uploaded scenarios
    DevBuf<int32_t> pool_dev;
    DevBuf<int32_t> fill_ctl;  // [2] K4's tick and finished-workgroup count
    DevBuf<int64_t> clock;     // [1] the step clock (K1 advances it)
    uint64_t seed = 0;
    bool reset_done = false;
    uint64_t* stamps = nullptr;  // diagnostic builds (D2D_STAMPS) only; the caller's buffer
    bool rc_dirty = true;        // scenarios changed since the reset cache was last dropped
    uint64_t n_steps = 0;        // d2d_step calls (fill cadence)
    d2d_curriculum cur{};        // fresh mode: generator parameters
    uint64_t fresh_seed = 0;
    bool fresh_seeded = false;
    int32_t generation = 0;        // bumped whenever captured graphs' pointers go stale
    std::vector<double> scn_cost;  // relative step cost per scenario (d2d_set_scenario_costs)
    // buffers were replaced: captured graphs point at the old ones, cached reset observations belong to them
    void stale() {
        generation += 1;
        rc_dirty = true;
    }
};

namespace {

bool fresh_mode(const d2d_t* h) { return h->cfg.scn_pool == 2; }

// the single place that flattens the handle into the kernels' arguments
StepArgs make_args(const d2d_t* h) {
    const Layout& L = h->lay;
    StepArgs a{};
    a.n = h->n;
    a.ns = L.ns;
    a.n_scn = h->tab.n_scn;
    a.st = L.st.get();
    a.ist = L.ist.get();
    a.acc = L.acc.get();
    a.scn = h->tab.scn.get();
    a.brt = h->tab.brt.get();  // (null in fresh curriculum mode: docs/DESIGN_HISTORY.md "Round 4")
    a.env_scn = h->env_scn.get();
    a.pool_base = h->pool_dev.get();
    a.pool_n = h->pool_n;
    a.fill_ctl = h->fill_ctl.get();
    a.fill_every = FILL_EVERY;
    a.fill_force = 0;
    a.cfg = h->cfg;
    a.damping_dt = std::pow(h->cfg.damping, 1.0 / 60.0);
    a.seed = h->seed;
    a.stamps = h->stamps;
    a.rc_obs = L.rc_obs.get();
    a.rc_rfl = L.rc_rfl.get();
    a.rc_tag = L.rc_tag.get();
    a.lane_env = L.lane_env.get();
    a.wg_scn = L.wg_scn.get();
    a.scn_tag = h->fresh.scn_tag.get();
    a.clock = h->clock.get();
    if (fresh_mode(h) && h->fresh.queue) {
        a.fq = h->fresh.queue.get();
        a.fqc = h->fresh.words();
        a.fq_mask = (uint32_t)h->fresh.ring - 1u;
    }
    return a;
}

constexpr int GEN_GRID = 2048;  // K5b workgroups
// K5: the fresh curriculum's scenario slots (restore: every slot from its recipe), on `stream`
hipError_t fresh_regen(d2d_t* h, hipStream_t stream, bool restore = false, bool queued = false) {
    FreshArgs f{};
    f.n = h->n;
    f.ist = h->lay.ist.get();
    f.env_scn = h->env_scn.get();
    f.cur = h->cur;
    f.W = h->cfg.screen_w;
    f.H = h->cfg.screen_h;
    f.seed = h->seed;
    f.env_id_base = (uint32_t)h->cfg.env_id_base;
    f.abi = h->tab.abi.get();
    f.scn = reinterpret_cast<d2d::ScnR*>(h->tab.scn.get());  // (fresh mode: tab.rm)
    f.tag = h->fresh.scn_tag.get();
    f.gclk = h->fresh.gclk.get();
    f.clock = h->clock.get();
    f.queue = h->fresh.queue.get();
    f.ring = h->fresh.words();
    f.mask = (uint32_t)h->fresh.ring - 1u;
    f.scan = queued ? 0 : 1;
    f.restore = restore ? 1 : 0;
#ifdef D2D_GEN_STAMPS
    f.stamps = h->stamps;
#endif
    const int items = restore ? 2 * h->n : h->n;
    if (!queued) hipLaunchKernelGGL(d2d_fresh_scan_kernel, dim3((items + 255) / 256), dim3(256), 0, stream, f);
    // one wave per queued slot: ~800 per step at 65 536 envs stepped with random actions (the items
    // of a step all run at once); a reset queues every env (the grid's workgroups then take several)
    hipLaunchKernelGGL(d2d_fresh_gen_kernel, dim3(std::min(items, GEN_GRID)), dim3(64), 0, stream, f);
    hipError_t e = hipGetLastError();
    // after a K1, K5b itself leaves the next tail (FreshRing: no launch; the round-4 clear kernel
    // after every K5b cost 5.5 us per step); after a scan, both tails to the head
    if (e != hipSuccess || queued) return e;
    hipLaunchKernelGGL(d2d_fresh_tail_kernel, dim3(1), dim3(64), 0, stream, f.ring);
    return hipGetLastError();
}
size_t ring_size(size_t slots) {  // FreshRing: a power of two holding every slot
    size_t r = 64;
    while (r < slots) r <<= 1;
    return r;
}

// Table placement: the one decision of where the kernels read the scenario table from, and so the
// table's layout (d2d_device.h ScnF / ScnR) and the K1 / K2 / K4 instantiations to launch.  The setters
// build the table in the layout it names; the launchers launch what it names.
using StepKernel = void (*)(StepArgs);
// K1 [LDS][LTAB][S3]; <false, true, *> is never chosen and not instantiated
constexpr StepKernel K1[2][2][2] = {
    {{d2d_step_kernel<false, false, false>, d2d_step_kernel<false, false, true>}, {nullptr, nullptr}},
    {{d2d_step_kernel<true, false, false>, d2d_step_kernel<true, false, true>},
     {d2d_step_kernel<true, true, false>, d2d_step_kernel<true, true, true>}}};
constexpr StepKernel K1_GROUPED[2] = {d2d_step_grouped_kernel<false>, d2d_step_grouped_kernel<true>};  // [S3]
constexpr StepKernel K2[2][2] = {{d2d_reset_kernel<false, false>, d2d_reset_kernel<false, true>},  // [LDS][RM]
                                 {d2d_reset_kernel<true, false>, d2d_reset_kernel<true, true>}};
constexpr StepKernel K4[2][2] = {{d2d_fill_kernel<false, false>, d2d_fill_kernel<false, true>},  // [LDS][RM]
                                 {d2d_fill_kernel<true, false>, d2d_fill_kernel<true, true>}};
static_assert(sizeof(d2d::ScnF) + sizeof(d2d::BtHot) + sizeof(K1Shared) <= K1_LDS_BUDGET, "grouped K1 LDS");
static_assert(sizeof(K1Shared) + K1_KN_BYTES <= K1_LDS_BUDGET, "K1 LDS with the staged knots");
struct Placement {
    bool rm;               // ScnR: K1 reads the table from global memory.  ScnF: it is staged in LDS
    const StepKernel* k1;  // [S3]
    StepKernel k2, k4;
    size_t k1_lds, k2_lds, k4_lds;  // dynamic LDS
};
size_t scn_size(bool rm) { return rm ? sizeof(d2d::ScnR) : sizeof(d2d::ScnF); }
// fresh: the fresh curriculum; grouped: the scenario-grouped slot layout; n_total: table entries;
// brt: the table has golden-march tables
Placement place(bool fresh, bool grouped, size_t n_total, bool brt) {
    Placement p{};
    const size_t scnf = sizeof(d2d::ScnF) * n_total, hot = sizeof(d2d::BtHot) * n_total;
    // ScnR exactly when K1 will read the table from global memory: the fresh curriculum, and tables
    // too big to stage (pools) unless the map is grouped (a grouped workgroup stages only its own scenarios)
    p.rm = fresh || (!grouped && scnf + sizeof(K1Shared) > K1_LDS_BUDGET);
    if (grouped) {
        p.k1 = K1_GROUPED;
        p.k1_lds = sizeof(d2d::ScnF) + sizeof(d2d::BtHot);
    } else if (p.rm) {
        // the plain search's staged knots only without golden-march tables (fresh curriculum);
        // a pool's tables take the table path, which never reads them
        p.k1 = K1[0][0];
        p.k1_lds = brt ? 0 : K1_KN_BYTES;
    } else {
        const bool ltab = brt && scnf + hot + sizeof(K1Shared) <= K1_LDS_BUDGET;  // the probe tables fit too
        p.k1 = K1[1][ltab];
        p.k1_lds = scnf + (ltab ? hot : 0);
    }
    // K2 and K4 stage the whole table when it fits; K4's dynamic LDS is padded to K1's per-workgroup
    // LDS, so K4 is resident 4 per CU as K1 (d2d_fill_kernel)
    const size_t table = scn_size(p.rm) * n_total;
    const size_t pad = sizeof(d2d::ScnF) + sizeof(d2d::BtHot) + sizeof(K1Shared) - 2048;
    const bool lds = table <= K2_LDS_BUDGET;
    p.k2 = K2[lds][p.rm];
    p.k2_lds = lds ? table : 0;
    p.k4 = K4[lds][p.rm];
    p.k4_lds = lds ? std::max(table, pad) : pad;
    return p;
}
Placement place(const d2d_t* h) {
    return place(fresh_mode(h), h->lay.grouped(), (size_t)h->tab.n_scn, h->tab.brt != nullptr);
}
void launch(StepKernel k, unsigned grid, int threads, size_t lds, hipStream_t stream, const StepArgs& a) {
    hipLaunchKernelGGL(k, dim3(grid), dim3(threads), lds, stream, a);
}

unsigned char* scn_at(const d2d_t* h, size_t k) { return h->tab.scn.get() + k * scn_size(h->tab.rm); }
// What is wrong with a scenario record, or null; entries with use[k] false are not looked at.
const char* scn_invalid(const d2d_scn* s, size_t n, const std::vector<bool>* use = nullptr) {
    for (size_t k = 0; k < n; ++k) {
        if (use && !(*use)[k]) continue;
        if (s[k].n_wps < 3 || s[k].n_wps > D2D_MAX_WPS) return "n_wps out of range [3, D2D_MAX_WPS]";
        if (s[k].n_circles < 0 || s[k].n_circles > D2D_MAX_CIRCLES) return "n_circles out of range [0, D2D_MAX_CIRCLES]";
    }
    return nullptr;
}
bool map_in_range(const int32_t* env_scn, int n, int n_scn) {
    return std::all_of(env_scn, env_scn + n, [=](int32_t v) { return v >= 0 && v < n_scn; });
}
// host tables in either layout; entries with use(k) false stay zero.  False: a scenario scn_build refuses
template <class S>
bool build_tables_t(const d2d_scn* src, size_t n, std::vector<unsigned char>& out, const std::vector<bool>* use) {
    out.assign(n * sizeof(S), 0);
    for (size_t k = 0; k < n; ++k)
        if ((!use || (*use)[k]) && !d2d::scn_build(src[k], *reinterpret_cast<S*>(out.data() + k * sizeof(S))))
            return false;
    return true;
}
bool build_tables(bool rm, const d2d_scn* src, size_t n, std::vector<unsigned char>& out,
                  const std::vector<bool>* use = nullptr) {
    return rm ? build_tables_t<d2d::ScnR>(src, n, out, use) : build_tables_t<d2d::ScnF>(src, n, out, use);
}
void launch_brtab(bool rm, const void* scn, int n, d2d::BrTab* out) {
    const dim3 grid((2 * n + 63) / 64);
    if (rm) hipLaunchKernelGGL(d2d_brtab_kernel<d2d::ScnR>, grid, dim3(64), 0, 0, (const d2d::ScnR*)scn, n, out);
    else hipLaunchKernelGGL(d2d_brtab_kernel<d2d::ScnF>, grid, dim3(64), 0, 0, (const d2d::ScnF*)scn, n, out);
}

// K4: fill every cache entry that does not belong to its env's current episode, ordered on `stream`
hipError_t rc_fill(d2d_t* h, hipStream_t stream, bool force = false) {
    StepArgs a = make_args(h);
    a.fill_force = force ? 1 : 0;
    const Placement p = place(h);
    launch(p.k4, (unsigned)(h->lay.ns + FILL_SPB - 1) / FILL_SPB, BLOCK, p.k4_lds, stream, a);
    return hipGetLastError();
}
// drop every entry (new seed, counters or scenarios) and refill, ordered on `stream`
hipError_t rc_rebuild(d2d_t* h, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(h->lay.rc_tag.get(), 0xFF, sizeof(int32_t) * RC_SLOTS * (size_t)h->lay.ns, stream);
    if (e == hipSuccess) e = rc_fill(h, stream, true);
    if (e == hipSuccess) h->rc_dirty = false;
    return e;
}

// allocate a layout of n envs: identity (lanes empty) or grouped (lanes: slot -> env, ws: scenario
// per group); state zeroed, reset cache empty
hipError_t alloc_layout(Layout& L, int n, const std::vector<int32_t>& lanes, const std::vector<int32_t>& ws) {
    L = Layout{};
    L.ns = lanes.empty() ? n : (int)lanes.size();
    const size_t ns = (size_t)L.ns;
    hipError_t e;
    if ((e = dev_new(L.st, D2D_NSTATE * ns)) != hipSuccess || (e = dev_new(L.ist, D2D_NISTATE * ns)) != hipSuccess ||
        (e = dev_new(L.acc, D2D_NSTATS * ns)) != hipSuccess ||
        (e = dev_new(L.rc_obs, D2D_OBS_DIM * RC_SLOTS * ns)) != hipSuccess ||
        (e = dev_new(L.rc_rfl, RC_SLOTS * ns)) != hipSuccess || (e = dev_new(L.rc_tag, RC_SLOTS * ns, 0xFF)) != hipSuccess ||
        lanes.empty())
        return e;
    std::vector<int32_t> es((size_t)n, 0);
    for (size_t k = 0; k < lanes.size(); ++k)
        if (lanes[k] >= 0) es[(size_t)lanes[k]] = (int32_t)k;
    if ((e = dev_new(L.lane_env, ns, 0, lanes.data(), ns)) != hipSuccess ||
        (e = dev_new(L.wg_scn, ws.size(), 0, ws.data(), ws.size())) != hipSuccess)
        return e;
    return dev_new(L.env_slot, (size_t)n, 0, es.data(), (size_t)n);
}
// every env's state, flags and accumulators from layout `from` to layout `to` (stream-ordered)
template <typename T>
hipError_t permute(const T* src, int sstride, const int32_t* sslot, T* dst, int dstride, const int32_t* dslot, int nf,
                   int n, hipStream_t stream) {
    hipLaunchKernelGGL(d2d_permute_kernel<T>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, src, sstride, sslot,
                       dst, dstride, dslot, nf, n);
    return hipGetLastError();
}
hipError_t move_state(const Layout& from, const Layout& to, int n) {
    const int32_t *fs = from.env_slot.get(), *ts = to.env_slot.get();
    hipError_t e;
    if ((e = permute(from.st.get(), from.ns, fs, to.st.get(), to.ns, ts, D2D_NSTATE, n, 0)) != hipSuccess ||
        (e = permute(from.ist.get(), from.ns, fs, to.ist.get(), to.ns, ts, D2D_NISTATE, n, 0)) != hipSuccess ||
        (e = permute(from.acc.get(), from.ns, fs, to.acc.get(), to.ns, ts, D2D_NSTATS, n, 0)) != hipSuccess)
        return e;
    return hipDeviceSynchronize();
}
// Put the running batch into the slot layout (lanes, ws) -- the identity when lanes is empty: allocate,
// move every env's state across, swap the layouts, free the old one.  A failure leaves the handle as it was.
hipError_t relayout(d2d_t* h, const std::vector<int32_t>& lanes, const std::vector<int32_t>& ws) {
    Layout to;
    hipError_t e = alloc_layout(to, h->n, lanes, ws);
    if (e == hipSuccess) e = move_state(h->lay, to, h->n);
    if (e != hipSuccess) return e;
    std::swap(h->lay, to);
    h->stale();  // captured graphs hold the old layout's buffers; the reset cache starts empty
    return hipSuccess;
}
// one state array between the handle's slot order and the caller's env order (to_env: out of the
// handle); an array the caller did not pass is skipped
template <typename T>
hipError_t copy_state(const d2d_t* h, bool to_env, const T* src, T* dst, int nf, hipStream_t s) {
    if (!src || !dst) return hipSuccess;
    const Layout& L = h->lay;
    if (!L.grouped()) return hipMemcpyAsync(dst, src, sizeof(T) * (size_t)nf * (size_t)h->n, hipMemcpyDeviceToDevice, s);
    const int32_t *none = nullptr, *slot = L.env_slot.get();
    return to_env ? permute(src, L.ns, slot, dst, h->n, none, nf, h->n, s)
                  : permute(src, h->n, none, dst, L.ns, slot, nf, h->n, s);
}

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// d2d_group_layout / d2d_balanced_group_layout (cost null: the natural order)
int32_t group_layout(const char* who, int32_t n, const int32_t* env_scn, int32_t n_scn, const double* cost, int32_t n_cu,
                     int32_t* slot_env, int32_t* group_scn) {
    if (!map_in_range(env_scn, n, n_scn)) return fail(D2D_E_ARG, std::string(who) + ": env scenario index out of range"), -1;
    std::vector<int32_t> lanes, ws;
    make_groups(n, env_scn, lanes, ws);
    if (cost) balance_groups(n_cu, cost, n_scn, lanes, ws);
    std::copy(lanes.begin(), lanes.end(), slot_env);
    std::copy(ws.begin(), ws.end(), group_scn);
    return (int32_t)ws.size();
}

}  // namespace

extern "C" {

int32_t d2d_abi_version(void) { return D2D_ABI_VERSION; }
const char* d2d_last_error(void) { return g_err.c_str(); }

int32_t d2d_create(const d2d_cfg* cfg, int32_t n_envs, int32_t device, d2d_t** out) {
    if (!cfg || !out || n_envs <= 0) return fail(D2D_E_ARG, "d2d_create: null cfg/out or n_envs <= 0");
    if (cfg->n_steps <= 0) return fail(D2D_E_ARG, "d2d_create: n_steps must be > 0");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    if (device < 0 || device >= ndev) return fail(D2D_E_ARG, "d2d_create: bad device index");
    DeviceGuard g(device);
    std::unique_ptr<d2d_t> h(new (std::nothrow) d2d_t());
    if (!h) return fail(D2D_E_NOMEM, "d2d_create: host allocation failed");
    h->cfg = *cfg;
    h->n = n_envs;
    h->device = device;
    if (hipDeviceGetAttribute(&h->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) h->n_cu = 256;
    if ((e = dev_new(h->env_scn, (size_t)n_envs)) != hipSuccess || (e = dev_new(h->pool_dev, 1)) != hipSuccess ||
        (e = dev_new(h->fill_ctl, 2)) != hipSuccess || (e = dev_new(h->clock, 1)) != hipSuccess ||
        (e = alloc_layout(h->lay, n_envs, {}, {})) != hipSuccess)
        return hip_fail(e, "d2d_create: hipMalloc");
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "d2d_create: memset");
    *out = h.release();
    return D2D_OK;
}

void d2d_destroy(d2d_t* h) {
    if (!h) return;
    DeviceGuard g(h->device);
    delete h;
}

int32_t d2d_n_envs(const d2d_t* h) { return h ? h->n : -1; }

#if defined(D2D_STAMPS) || defined(D2D_GEN_STAMPS)
// diagnostic builds only: K1 writes 8 s_memtime stamps per wave into buf ([n_blocks*4][8] u64)
int32_t d2d_debug_stamps(d2d_t* h, uint64_t* buf) {
    if (!h) return fail(D2D_E_ARG, "d2d_debug_stamps: null handle");
    h->stamps = buf;
    return D2D_OK;
}
#endif
#ifdef D2D_BSTAMP
// diagnostic builds only: the Brent-step stamps (d2d_device.h, D2D_BSTAMP): clear = 1 zeroes them,
// else copies [1024][64][8] u64 into out
int32_t d2d_debug_bstamps(uint64_t* out, int32_t clear) {
    void* p = nullptr;
    hipError_t e = hipGetSymbolAddress(&p, HIP_SYMBOL(d2d_bst));
    if (e == hipSuccess) e = clear ? hipMemset(p, 0, sizeof(uint64_t) * BST_N)
                                   : hipMemcpy(out, p, sizeof(uint64_t) * BST_N, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e == hipSuccess ? D2D_OK : hip_fail(e, "d2d_debug_bstamps");
}
#endif

int32_t d2d_set_scenarios(d2d_t* h, const d2d_scn* scns, int32_t n_scn, const int32_t* env_scn_host) {
    if (!h || !scns || n_scn <= 0) return fail(D2D_E_ARG, "d2d_set_scenarios: null handle/scenarios or n_scn <= 0");
    if (fresh_mode(h)) return fail(D2D_E_ARG, "d2d_set_scenarios: fresh curriculum mode (cfg.scn_pool = 2) uses d2d_set_curriculum");
    if (const char* why = scn_invalid(scns, (size_t)n_scn)) return fail(D2D_E_ARG, std::string("d2d_set_scenarios: ") + why);
    if (env_scn_host && !map_in_range(env_scn_host, h->n, n_scn))
        return fail(D2D_E_ARG, "d2d_set_scenarios: env scenario index out of range");
    // validate and build everything before touching the handle: a bad scenario leaves it as it was
    // pool mode: room for a second pool half (d2d_refresh_pool), zero until the first refresh
    const size_t T = (size_t)n_scn * (h->cfg.scn_pool ? 2 : 1);
    // slot layout: grouped for a static mixed map (pool mode redraws scenarios at every reset)
    const bool grouped = env_scn_host && n_scn > 1 && !h->cfg.scn_pool;
    ScnTables tab;
    tab.n_scn = (int)T;
    tab.rm = place(false, grouped, T, true).rm;
    std::vector<unsigned char> host;
    if (!build_tables(tab.rm, scns, (size_t)n_scn, host))
        return fail(D2D_E_ARG, "d2d_set_scenarios: us[n_wps-2] - us[n_wps-3] must exceed 0.001");
    DeviceGuard g(h->device);
    hipError_t e;
    if ((e = dev_new(tab.scn, scn_size(tab.rm) * T, 0, host.data(), host.size())) != hipSuccess)
        return hip_fail(e, "hipMalloc scn");
    // pool mode keeps the ABI records for checkpoints / readback
    if (h->cfg.scn_pool && (e = dev_new(tab.abi, T, 0, scns, (size_t)n_scn)) != hipSuccess) return hip_fail(e, "hipMalloc abi");
    // golden-march tables: forced searches on the device (same arithmetic as the step kernels)
    if ((e = dev_new(tab.brt, T)) != hipSuccess) return hip_fail(e, "hipMalloc brt");
    launch_brtab(tab.rm, tab.scn.get(), n_scn, tab.brt.get());
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "d2d_brtab_kernel launch");
    if ((e = hipMemset(h->pool_dev.get(), 0, sizeof(int32_t))) != hipSuccess) return hip_fail(e, "hipMemset pool");
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "d2d_brtab_kernel");
    std::vector<int32_t> lanes, ws;
    if (grouped) {
        make_groups(h->n, env_scn_host, lanes, ws);
        if ((int)h->scn_cost.size() == n_scn) balance_groups(h->n_cu, h->scn_cost.data(), n_scn, lanes, ws);
    }
    // commit: the current state moves into the new layout (the last step that can fail with the
    // handle intact), then the handle takes the new scenarios
    if (grouped || h->lay.grouped()) {
        if ((e = relayout(h, lanes, ws)) != hipSuccess) return hip_fail(e, "d2d_set_scenarios: layout");
    } else {
        h->stale();  // the old tables are freed: captured graphs point at them
    }
    h->tab = std::move(tab);
    h->pool_base = 0;
    h->pool_n = n_scn;
    h->pool_valid = 1;
    if ((int)h->scn_cost.size() != n_scn) h->scn_cost.assign((size_t)n_scn, 1.0);
    e = env_scn_host ? hipMemcpy(h->env_scn.get(), env_scn_host, sizeof(int32_t) * (size_t)h->n, hipMemcpyHostToDevice)
                     : hipMemset(h->env_scn.get(), 0, sizeof(int32_t) * (size_t)h->n);
    if (e != hipSuccess) {
        // the env -> scenario map is unknown: no step or reset until the next d2d_set_scenarios
        h->tab.n_scn = 0;
        h->reset_done = false;
        return hip_fail(e, "d2d_set_scenarios: env_scn upload");
    }
    return D2D_OK;
}

int32_t d2d_set_scenario_costs(d2d_t* h, const double* cost, int32_t n_scn) {
    if (!h || !cost) return fail(D2D_E_ARG, "d2d_set_scenario_costs: null argument");
    if (h->cfg.scn_pool || n_scn != h->tab.n_scn) return fail(D2D_E_ARG, "d2d_set_scenario_costs: one cost per scenario (test mode)");
    for (int k = 0; k < n_scn; ++k)
        if (!(cost[k] >= 0.0)) return fail(D2D_E_ARG, "d2d_set_scenario_costs: costs must be >= 0");
    DeviceGuard g(h->device);
    hipError_t e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "d2d_set_scenario_costs: sync");
    if (h->lay.grouped()) {
        // grouped layout: deal the groups over the CUs by the new costs (balance_groups); the state
        // moves into the renumbered layout, the reset cache refills
        std::vector<int32_t> es((size_t)h->n);
        if ((e = hipMemcpy(es.data(), h->env_scn.get(), sizeof(int32_t) * (size_t)h->n, hipMemcpyDeviceToHost)) != hipSuccess)
            return hip_fail(e, "d2d_set_scenario_costs: env_scn");
        std::vector<int32_t> lanes, ws;
        make_groups(h->n, es.data(), lanes, ws);
        balance_groups(h->n_cu, cost, n_scn, lanes, ws);
        if ((e = relayout(h, lanes, ws)) != hipSuccess) return hip_fail(e, "d2d_set_scenario_costs: layout");
    }
    h->scn_cost.assign(cost, cost + n_scn);
    return D2D_OK;
}

int32_t d2d_get_group_layout(d2d_t* h, int32_t* slot_env, int32_t* group_scn) {
    if (!h) return fail(D2D_E_ARG, "d2d_get_group_layout: null handle"), -1;
    const Layout& L = h->lay;
    if (!L.grouped()) return 0;
    if (!slot_env || !group_scn) return fail(D2D_E_ARG, "d2d_get_group_layout: null output"), -1;
    DeviceGuard g(h->device);
    hipError_t e;
    if ((e = hipDeviceSynchronize()) != hipSuccess ||
        (e = hipMemcpy(slot_env, L.lane_env.get(), sizeof(int32_t) * (size_t)L.ns, hipMemcpyDeviceToHost)) != hipSuccess ||
        (e = hipMemcpy(group_scn, L.wg_scn.get(), sizeof(int32_t) * (size_t)L.n_groups(), hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_fail(e, "d2d_get_group_layout"), -1;
    return L.n_groups();
}

int32_t d2d_reset(d2d_t* h, const uint8_t* mask_dev, uint64_t seed, float* obs_dev, void* stream) {
    if (!h) return fail(D2D_E_ARG, "d2d_reset: null handle");
    if (h->tab.n_scn <= 0) return fail(D2D_E_STATE, "d2d_reset: call d2d_set_scenarios first");
    DeviceGuard g(h->device);
    hipError_t e;
    const hipStream_t rs = (hipStream_t)stream;
    if (fresh_mode(h) && mask_dev && (!h->fresh_seeded || h->fresh_seed != seed))
        return fail(D2D_E_ARG, "d2d_reset: fresh curriculum -- a masked reset must keep the seed of the "
                               "previous full reset");
    h->seed = seed;
    if (fresh_mode(h)) {
        // scenarios are keyed by the seed: a new seed drops every slot; then the slots of the
        // episodes this reset starts.  (A masked reset cannot change the seed, checked above: the
        // envs it leaves running would keep old-seed scenarios no recipe (key, clock) regenerates.)
        if (!h->fresh_seeded || h->fresh_seed != seed) {
            if ((e = hipMemsetAsync(h->fresh.scn_tag.get(), 0xFF, sizeof(int32_t) * 2 * (size_t)h->n, rs)) != hipSuccess)
                return hip_fail(e, "d2d_reset: fresh slots");
            h->fresh_seed = seed;
            h->fresh_seeded = true;
        }
        if ((e = fresh_regen(h, rs)) != hipSuccess) return hip_fail(e, "d2d_reset: fresh scenarios");
    }
    StepArgs a = make_args(h);
    a.obs = obs_dev;
    a.mask = mask_dev;
    const Placement p = place(h);
    launch(p.k2, (unsigned)(h->lay.ns + BLOCK - 1) / BLOCK, BLOCK, p.k2_lds, rs, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "d2d_reset launch");
    if (fresh_mode(h) && (e = fresh_regen(h, rs)) != hipSuccess) return hip_fail(e, "d2d_reset: fresh scenarios");
    // cached next-reset observations depend on the seed and the episode counters: drop and refill
    if ((e = rc_rebuild(h, rs)) != hipSuccess) return hip_fail(e, "d2d_reset: cache rebuild");
    h->reset_done = true;
    return D2D_OK;
}

int32_t d2d_step(d2d_t* h, const float* act_dev, float* obs_dev, float* rew_dev, uint8_t* term_dev,
                 uint8_t* trunc_dev, float* info_dev, float* term_obs_dev, void* stream) {
    if (!h || !act_dev || !obs_dev || !rew_dev || !term_dev || !trunc_dev)
        return fail(D2D_E_ARG, "d2d_step: null handle or required buffer");
    if (h->tab.n_scn <= 0 || !h->reset_done) return fail(D2D_E_STATE, "d2d_step: call d2d_set_scenarios and d2d_reset first");
    if (((uintptr_t)act_dev & 7u) != 0) return fail(D2D_E_ARG, "d2d_step: act_dev must be 8-byte aligned");
    DeviceGuard g(h->device);
    hipError_t e;
    const hipStream_t ss = (hipStream_t)stream;
    if (h->rc_dirty && (e = rc_rebuild(h, ss)) != hipSuccess) return hip_fail(e, "d2d_step: cache rebuild");
    StepArgs a = make_args(h);
    a.act = act_dev;
    a.obs = obs_dev;
    a.rew = rew_dev;
    a.term = term_dev;
    a.trunc = trunc_dev;
    a.info = info_dev;
    a.tobs = term_obs_dev;
    const Placement p = place(h);
    // the three-way table re-check pays when the SIMDs have idle issue slots (at most one K1
    // workgroup per CU: 4 096 / 16 384 envs -4 %), not at full load (65 536 envs +3.6 %)
    const int nwg = h->lay.grouped() ? h->lay.n_groups() : (h->n + EPB - 1) / EPB;
    const bool s3 = nwg <= std::max(h->n_cu, 1);
    launch(p.k1[s3], (unsigned)nwg, K1_THREADS, p.k1_lds, ss, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "d2d_step launch");
    if (fresh_mode(h) && (e = fresh_regen(h, ss, false, h->cfg.auto_reset != 0)) != hipSuccess)
        return hip_fail(e, "d2d_step: fresh scenarios");
    if (h->cfg.auto_reset && ++h->n_steps % FILL_PERIOD == 0) {
        // K4's cadence.  A step being captured into a graph launches K4 every FILL_PERIOD steps and
        // lets the device tick pick every FILL_EVERY-th launch to fill, so replays keep the cadence
        // whatever the graph's length; an eager step launches only the filling launches (every
        // FILL_PERIOD x FILL_EVERY steps), saving the two launches per period that would find the tick
        // says "skip" (~4 us each).  Either way an entry is an optimisation: a reset whose entry is
        // missing computes the same observation in K1.
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if ((e = hipStreamIsCapturing(ss, &cs)) != hipSuccess) return hip_fail(e, "d2d_step: capture query");
        if (cs != hipStreamCaptureStatusNone) {
            if ((e = rc_fill(h, ss)) != hipSuccess) return hip_fail(e, "d2d_step: cache fill");
        } else if (h->n_steps % (FILL_PERIOD * FILL_EVERY) == 0) {
            if ((e = rc_fill(h, ss, true)) != hipSuccess) return hip_fail(e, "d2d_step: cache fill");
        }
    }
    return D2D_OK;
}

int32_t d2d_get_state(d2d_t* h, double* state_dev, int32_t* istate_dev, void* stream) {
    if (!h) return fail(D2D_E_ARG, "d2d_get_state: null handle");
    DeviceGuard g(h->device);
    hipError_t e;
    if ((e = copy_state<double>(h, true, h->lay.st.get(), state_dev, D2D_NSTATE, (hipStream_t)stream)) != hipSuccess ||
        (e = copy_state<int32_t>(h, true, h->lay.ist.get(), istate_dev, D2D_NISTATE, (hipStream_t)stream)) != hipSuccess)
        return hip_fail(e, "d2d_get_state");
    return D2D_OK;
}

int32_t d2d_set_state(d2d_t* h, const double* state_dev, const int32_t* istate_dev, void* stream) {
    if (!h) return fail(D2D_E_ARG, "d2d_set_state: null handle");
    if (h->tab.n_scn <= 0) return fail(D2D_E_STATE, "d2d_set_state: call d2d_set_scenarios first");
    DeviceGuard g(h->device);
    hipError_t e;
    const hipStream_t s = (hipStream_t)stream;
    if ((e = copy_state<double>(h, false, state_dev, h->lay.st.get(), D2D_NSTATE, s)) != hipSuccess ||
        (e = copy_state<int32_t>(h, false, istate_dev, h->lay.ist.get(), D2D_NISTATE, s)) != hipSuccess)
        return hip_fail(e, "d2d_set_state");
    if (fresh_mode(h) && (e = fresh_regen(h, s)) != hipSuccess) return hip_fail(e, "d2d_set_state: fresh scenarios");
    if ((e = rc_rebuild(h, s)) != hipSuccess) return hip_fail(e, "d2d_set_state: cache rebuild");
    h->reset_done = true;
    return D2D_OK;
}

int32_t d2d_refresh_pool(d2d_t* h, const d2d_scn* scns, int32_t n_scn) {
    if (!h || !scns) return fail(D2D_E_ARG, "d2d_refresh_pool: null handle/scenarios");
    if (h->cfg.scn_pool != 1) return fail(D2D_E_ARG, "d2d_refresh_pool: pool mode only (cfg.scn_pool = 1)");
    if (h->tab.n_scn <= 0) return fail(D2D_E_STATE, "d2d_refresh_pool: call d2d_set_scenarios first");
    if (n_scn != h->pool_n) return fail(D2D_E_ARG, "d2d_refresh_pool: n_scn must equal the pool size");
    std::vector<unsigned char> tab;
    if (scn_invalid(scns, (size_t)n_scn) || !build_tables(h->tab.rm, scns, (size_t)n_scn, tab))
        return fail(D2D_E_ARG, "d2d_refresh_pool: invalid scenario");
    DeviceGuard g(h->device);
    hipError_t e;
    const size_t P = (size_t)n_scn;
    const int half = h->pool_base == 0 ? n_scn : 0;
    // the half about to be overwritten must not hold a running episode (one that started before the
    // previous refresh): episodes last at most cfg.n_steps steps, so refreshes further apart are safe
    std::vector<int32_t> es((size_t)h->n);
    if ((e = hipDeviceSynchronize()) != hipSuccess ||  // in-flight steps may still draw from the old half
        (e = hipMemcpy(es.data(), h->env_scn.get(), sizeof(int32_t) * es.size(), hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_fail(e, "d2d_refresh_pool: read env_scn");
    int busy = 0;
    for (int32_t v : es) busy += (v >= half && v < half + n_scn);
    if (busy)
        return fail(D2D_E_STATE, "d2d_refresh_pool: " + std::to_string(busy) +
                                     " envs still run episodes from the pool before the previous refresh");
    d2d_scn* abi = h->tab.abi.get();
    d2d::BrTab* brt = h->tab.brt.get();
    if ((e = hipMemcpy(scn_at(h, half), tab.data(), tab.size(), hipMemcpyHostToDevice)) != hipSuccess ||
        (abi && (e = hipMemcpy(abi + half, scns, P * sizeof(d2d_scn), hipMemcpyHostToDevice)) != hipSuccess) ||
        (e = hipMemset(brt + half, 0, P * sizeof(d2d::BrTab))) != hipSuccess)
        return hip_fail(e, "d2d_refresh_pool: upload");
    launch_brtab(h->tab.rm, scn_at(h, half), n_scn, brt + half);
    if ((e = hipGetLastError()) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
        return hip_fail(e, "d2d_refresh_pool: d2d_brtab_kernel");
    if ((e = hipMemcpy(h->pool_dev.get(), &half, sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess)
        return hip_fail(e, "d2d_refresh_pool: switch");
    h->pool_base = half;
    h->pool_valid |= (half == 0) ? 1 : 2;
    // cached next-episode observations were drawn from the old half: drop and refill now (a
    // captured graph replays d2d_step's kernels without the host-side rebuild check)
    if ((e = rc_rebuild(h, nullptr)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
        return hip_fail(e, "d2d_refresh_pool: cache rebuild");
    return D2D_OK;
}

int32_t d2d_get_env_scenarios(d2d_t* h, int32_t* env_scn_dev, void* stream) {
    if (!h || !env_scn_dev) return fail(D2D_E_ARG, "d2d_get_env_scenarios: null handle/out");
    DeviceGuard g(h->device);
    hipError_t e = hipMemcpyAsync(env_scn_dev, h->env_scn.get(), sizeof(int32_t) * (size_t)h->n, hipMemcpyDeviceToDevice,
                                  (hipStream_t)stream);
    if (e != hipSuccess) return hip_fail(e, "d2d_get_env_scenarios");
    return D2D_OK;
}

int32_t d2d_set_env_scenarios(d2d_t* h, const int32_t* env_scn_dev, void* stream) {
    if (!h || !env_scn_dev) return fail(D2D_E_ARG, "d2d_set_env_scenarios: null handle/map");
    if (h->cfg.scn_pool != 1)
        return fail(D2D_E_ARG, "d2d_set_env_scenarios: pool mode only (a static map changes with d2d_set_scenarios; "
                               "fresh curriculum slots are restored by d2d_fresh_recipes)");
    if (h->tab.n_scn <= 0) return fail(D2D_E_STATE, "d2d_set_env_scenarios: call d2d_set_scenarios first");
    DeviceGuard g(h->device);
    const hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> m((size_t)h->n);
    hipError_t e = hipMemcpyAsync(m.data(), env_scn_dev, sizeof(int32_t) * m.size(), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "d2d_set_env_scenarios: read map");
    for (int32_t v : m) {
        if (v < 0 || v >= h->tab.n_scn) return fail(D2D_E_ARG, "d2d_set_env_scenarios: scenario index out of range");
        if (!(h->pool_valid & (v >= h->pool_n ? 2 : 1)))
            return fail(D2D_E_ARG, "d2d_set_env_scenarios: index into a pool half that holds no scenarios");
    }
    if ((e = hipMemcpyAsync(h->env_scn.get(), m.data(), sizeof(int32_t) * m.size(), hipMemcpyHostToDevice, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
        return hip_fail(e, "d2d_set_env_scenarios");
    return D2D_OK;
}

int32_t d2d_pool_state(d2d_t* h, int32_t* active_base, int32_t* valid_mask) {
    if (!h || !active_base || !valid_mask) return fail(D2D_E_ARG, "d2d_pool_state: null argument");
    if (h->cfg.scn_pool != 1 || h->tab.n_scn <= 0) return fail(D2D_E_STATE, "d2d_pool_state: pool mode with scenarios only");
    *active_base = h->pool_base;
    *valid_mask = h->pool_valid;
    return D2D_OK;
}

int32_t d2d_restore_pool(d2d_t* h, const d2d_scn* scns, int32_t n_total, int32_t active_base, int32_t valid_mask) {
    if (!h || !scns) return fail(D2D_E_ARG, "d2d_restore_pool: null argument");
    if (h->cfg.scn_pool != 1 || h->tab.n_scn <= 0) return fail(D2D_E_STATE, "d2d_restore_pool: pool mode with scenarios only");
    const int P = h->pool_n;
    if (n_total != 2 * P) return fail(D2D_E_ARG, "d2d_restore_pool: n_total must be twice the pool size");
    if (active_base != 0 && active_base != P) return fail(D2D_E_ARG, "d2d_restore_pool: active_base must be 0 or pool_n");
    if (!(valid_mask & (active_base ? 2 : 1)) || (valid_mask & ~3))
        return fail(D2D_E_ARG, "d2d_restore_pool: the active half must be valid");
    std::vector<bool> use((size_t)n_total);
    for (int k = 0; k < n_total; ++k) use[(size_t)k] = (valid_mask & (k >= P ? 2 : 1)) != 0;
    std::vector<unsigned char> tab;
    if (scn_invalid(scns, (size_t)n_total, &use) || !build_tables(h->tab.rm, scns, (size_t)n_total, tab, &use))
        return fail(D2D_E_ARG, "d2d_restore_pool: invalid scenario");
    const size_t sz = scn_size(h->tab.rm);
    d2d_scn* abi = h->tab.abi.get();
    d2d::BrTab* brt = h->tab.brt.get();
    DeviceGuard g(h->device);
    hipError_t e;
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "d2d_restore_pool: sync");
    for (int half = 0; half < 2; ++half) {
        const size_t o = (size_t)half * P;
        if (!(valid_mask & (1 << half))) {
            if ((e = hipMemset(scn_at(h, o), 0, P * sz)) != hipSuccess ||
                (e = hipMemset(abi + o, 0, P * sizeof(d2d_scn))) != hipSuccess ||
                (e = hipMemset(brt + o, 0, P * sizeof(d2d::BrTab))) != hipSuccess)
                return hip_fail(e, "d2d_restore_pool: clear");
            continue;
        }
        if ((e = hipMemcpy(scn_at(h, o), tab.data() + o * sz, P * sz, hipMemcpyHostToDevice)) != hipSuccess ||
            (e = hipMemcpy(abi + o, scns + o, P * sizeof(d2d_scn), hipMemcpyHostToDevice)) != hipSuccess ||
            (e = hipMemset(brt + o, 0, P * sizeof(d2d::BrTab))) != hipSuccess)
            return hip_fail(e, "d2d_restore_pool: upload");
        launch_brtab(h->tab.rm, scn_at(h, o), P, brt + o);
        if ((e = hipGetLastError()) != hipSuccess) return hip_fail(e, "d2d_restore_pool: d2d_brtab_kernel");
    }
    if ((e = hipMemcpy(h->pool_dev.get(), &active_base, sizeof(int32_t), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipDeviceSynchronize()) != hipSuccess)
        return hip_fail(e, "d2d_restore_pool: switch");
    h->pool_base = active_base;
    h->pool_valid = valid_mask;
    h->rc_dirty = true;
    return D2D_OK;
}

int32_t d2d_set_curriculum(d2d_t* h, const d2d_curriculum* c) {
    if (!h || !c) return fail(D2D_E_ARG, "d2d_set_curriculum: null argument");
    if (!fresh_mode(h)) return fail(D2D_E_ARG, "d2d_set_curriculum: needs cfg.scn_pool = 2 (fresh curriculum)");
    if (c->n_wps < 4 || c->n_wps > D2D_MAX_WPS) return fail(D2D_E_ARG, "d2d_set_curriculum: n_wps out of range [4, D2D_MAX_WPS]");
    if (!(c->segment_length > 0.001)) return fail(D2D_E_ARG, "d2d_set_curriculum: segment_length must exceed 0.001");
    if (c->stage < 0 || c->stage > 5) return fail(D2D_E_ARG, "d2d_set_curriculum: stage must be 0 (schedule) or 1..5");
    if (c->random_path_spawn && (c->corner_lo < 1 || c->corner_hi > 4 || c->corner_lo > c->corner_hi))
        return fail(D2D_E_ARG, "d2d_set_curriculum: spawn corners must satisfy 1 <= lo <= hi <= 4");
    if (!(c->envs_total >= 1.0)) return fail(D2D_E_ARG, "d2d_set_curriculum: envs_total must be >= 1");
    DeviceGuard g(h->device);
    hipError_t e;
    const size_t S = 2 * (size_t)h->n;
    // the first curriculum of a handle builds its tables and slots, later ones keep them; the handle
    // takes them only once all of them exist
    const bool build = h->tab.n_scn != (int)S || !h->fresh.scn_tag;
    ScnTables tab;
    FreshSlots fr;
    if (build) {
        tab.n_scn = (int)S;
        tab.rm = place(true, false, S, false).rm;  // (read per lane from global memory; no golden-march tables)
        fr.ring = ring_size(S);
        if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "d2d_set_curriculum: sync");
        if ((e = dev_new(tab.scn, scn_size(tab.rm) * S)) != hipSuccess || (e = dev_new(tab.abi, S)) != hipSuccess ||
            (e = dev_new(fr.scn_tag, S)) != hipSuccess || (e = dev_new(fr.gclk, S)) != hipSuccess ||
            (e = dev_new(fr.queue, fr.ring + FR_WORDS)) != hipSuccess)
            return hip_fail(e, "d2d_set_curriculum: hipMalloc");
    }
    const FreshSlots& f = build ? fr : h->fresh;
    // the schedule restarts at c->sim_num0: sim_num = sim_num0 + clock * envs_total counts the steps
    // taken on THIS curriculum, not those since the handle was created
    if ((e = hipMemset(f.scn_tag.get(), 0xFF, sizeof(int32_t) * S)) != hipSuccess ||
        (e = hipMemset(h->clock.get(), 0, sizeof(int64_t))) != hipSuccess ||
        (e = hipMemset(f.words(), 0, sizeof(int32_t) * FR_WORDS)) != hipSuccess ||  // (FreshRing)
        (e = hipDeviceSynchronize()) != hipSuccess)
        return hip_fail(e, "d2d_set_curriculum: slots");
    if (build) {
        h->tab = std::move(tab);
        h->fresh = std::move(fr);
    }
    h->cur = *c;
    h->pool_n = 0;
    h->fresh_seeded = false;
    h->reset_done = false;  // every env starts over on the new curriculum (d2d_reset)
    h->stale();
    return D2D_OK;
}

int32_t d2d_fresh_recipes(d2d_t* h, int32_t* keys, int64_t* clocks, int64_t* clock, int32_t set) {
    if (!h || !keys || !clocks || !clock) return fail(D2D_E_ARG, "d2d_fresh_recipes: null argument");
    if (!fresh_mode(h) || !h->fresh.scn_tag) return fail(D2D_E_STATE, "d2d_fresh_recipes: call d2d_set_curriculum first");
    DeviceGuard g(h->device);
    hipError_t e;
    const size_t S = 2 * (size_t)h->n;
    int32_t* tag = h->fresh.scn_tag.get();
    int64_t* gclk = h->fresh.gclk.get();
    if ((e = hipDeviceSynchronize()) != hipSuccess) return hip_fail(e, "d2d_fresh_recipes: sync");
    if (!set) {
        if ((e = hipMemcpy(keys, tag, sizeof(int32_t) * S, hipMemcpyDeviceToHost)) != hipSuccess ||
            (e = hipMemcpy(clocks, gclk, sizeof(int64_t) * S, hipMemcpyDeviceToHost)) != hipSuccess ||
            (e = hipMemcpy(clock, h->clock.get(), sizeof(int64_t), hipMemcpyDeviceToHost)) != hipSuccess)
            return hip_fail(e, "d2d_fresh_recipes: read");
        return D2D_OK;
    }
    if (!h->fresh_seeded) return fail(D2D_E_STATE, "d2d_fresh_recipes: call d2d_reset (the seed) before restoring");
    if ((e = hipMemcpy(tag, keys, sizeof(int32_t) * S, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(gclk, clocks, sizeof(int64_t) * S, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(h->clock.get(), clock, sizeof(int64_t), hipMemcpyHostToDevice)) != hipSuccess)
        return hip_fail(e, "d2d_fresh_recipes: write");
    if ((e = fresh_regen(h, nullptr, true)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)
        return hip_fail(e, "d2d_fresh_recipes: regenerate");
    h->rc_dirty = true;
    return D2D_OK;
}

int32_t d2d_get_scenario_table(d2d_t* h, int32_t first, int32_t count, d2d_scn* out) {
    if (!h || !out || first < 0 || count < 0) return fail(D2D_E_ARG, "d2d_get_scenario_table: bad arguments");
    if (!h->tab.abi) return fail(D2D_E_STATE, "d2d_get_scenario_table: pool or fresh curriculum mode with scenarios only");
    if (first + count > h->tab.n_scn) return fail(D2D_E_ARG, "d2d_get_scenario_table: range beyond the table");
    DeviceGuard g(h->device);
    hipError_t e;
    if ((e = hipDeviceSynchronize()) != hipSuccess ||
        (e = hipMemcpy(out, h->tab.abi.get() + first, sizeof(d2d_scn) * (size_t)count, hipMemcpyDeviceToHost)) != hipSuccess)
        return hip_fail(e, "d2d_get_scenario_table");
    return D2D_OK;
}

int32_t d2d_generation(const d2d_t* h) { return h ? h->generation : -1; }

int32_t d2d_episode_stats(d2d_t* h, double* out_dev, int32_t clear, void* stream) {
    if (!h || !out_dev) return fail(D2D_E_ARG, "d2d_episode_stats: null handle/out");
    DeviceGuard g(h->device);
    double* acc = h->lay.acc.get();
    hipLaunchKernelGGL(d2d_stats_kernel, dim3(D2D_NSTATS), dim3(BLOCK), 0, (hipStream_t)stream, acc, h->lay.ns, out_dev,
                       clear, acc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "d2d_episode_stats launch");
    return D2D_OK;
}

int32_t d2d_group_layout(int32_t n, const int32_t* env_scn, int32_t n_scn, int32_t* slot_env, int32_t* group_scn) {
    if (n <= 0 || n_scn <= 0 || !env_scn || !slot_env || !group_scn)
        return fail(D2D_E_ARG, "d2d_group_layout: n, n_scn must be > 0 and pointers non-null"), -1;
    return group_layout("d2d_group_layout", n, env_scn, n_scn, nullptr, 0, slot_env, group_scn);
}

int32_t d2d_balanced_group_layout(int32_t n, const int32_t* env_scn, int32_t n_scn, const double* cost, int32_t n_cu,
                                  int32_t* slot_env, int32_t* group_scn) {
    if (n <= 0 || n_scn <= 0 || !env_scn || !cost || !slot_env || !group_scn || n_cu < 0)
        return fail(D2D_E_ARG, "d2d_balanced_group_layout: bad arguments"), -1;
    return group_layout("d2d_balanced_group_layout", n, env_scn, n_scn, cost, n_cu, slot_env, group_scn);
}

int32_t d2d_selftest(int32_t which, int64_t n, uint64_t seed, uint64_t* mismatches) {
    if (!mismatches || n < 0 || which < 0 || which > 2) return fail(D2D_E_ARG, "d2d_selftest: bad arguments");
    DevBuf<unsigned long long> bad;
    hipError_t e;
    if ((e = dev_new(bad, 1)) != hipSuccess) return hip_fail(e, "d2d_selftest alloc");
    hipLaunchKernelGGL(d2d_selftest_kernel, dim3(2048), dim3(256), 0, 0, which, (long long)n, seed, bad.get());
    e = hipGetLastError();
    unsigned long long h = 0;
    if (e == hipSuccess) e = hipMemcpy(&h, bad.get(), sizeof(h), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "d2d_selftest");
    *mismatches = (uint64_t)h;
    return D2D_OK;
}

}  // extern "C"
