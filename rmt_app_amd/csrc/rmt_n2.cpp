// C-ABI host side of the MI355X N2 integrator (see include/rmt_n2.h for the contract and the
// reference interfaces each entry point replaces).  Host code only: the device code is the
// template in kernels/*.inc (concatenated by embed.py in the order of kernels/ORDER), specialised by a generated prelude and compiled with hipRTC.
#include "rmt_n2.h"

#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

static const char* const k_template =
#include "n2_kernels_embed.h"
    ;
// the monitor's translation unit (monitor_kernels.inc): mechanism-independent, compiled on its own
static const char* const k_monitor_source =
#include "monitor_kernels_embed.h"
    ;
// the controller's translation unit (control_kernels.inc): mechanism-independent, compiled on its own
static const char* const k_control_source =
#include "control_kernels_embed.h"
    ;
// the fit's translation unit (fit_kernels.inc): mechanism-independent, compiled on its own
static const char* const k_fit_source =
#include "fit_kernels_embed.h"
    ;

static thread_local std::string g_err;

// workgroups per CU the single-evaluation kernel rmt_n2_rhs is launched with at most (it loops over the reactors): enough
// to fill every wave slot the kernel's registers allow (4 per SIMD at 256 threads), with a second set queued behind
#define RMT_N2_RHS_WGS_PER_CU 8
// calls of rmt_n2_rk4 that run the plain on-chip stepper alone after a cached launch lost half of its reactors to it
#define RMT_N2_PLAIN_LAUNCHES 8

static int fail(const char* fmt, ...) {
    char buf[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

#define HIP_OK(call)                                                                       \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess) return fail("%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// One device allocation and its size, freed with its owner.  reserve() is THE grow rule of every buffer that is created
// on first use or grows with a call: large enough - nothing; else wait for the stream (a launch in flight may still use
// the old buffer), free, allocate; a failure leaves the buffer empty.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    int reserve(hipStream_t stream, size_t need) {
        if (bytes >= need) return 0;
        if (p) {
            HIP_OK(hipStreamSynchronize(stream));
            release();
        }
        HIP_OK(hipMalloc(&p, need));
        bytes = need;
        return 0;
    }
    template <class T>
    T* as() const { return (T*)p; }
};

// (Kernel arguments name a buffer as `&buf.p`: the address of the device pointer, read at the launch.)
struct rmt_n2_handle {
    int S = 0, V = 0, NU = 0, N = 0, E = 0, fp32 = 0, block = 0, npt = 0, mode = 0, device = 0;
    int ros_nb = 0;                          // mesh nodes per workgroup of the stiff stepper (block, or block / 4 in the quad layout)
    size_t real_size = 8;
    hipModule_t module = nullptr;
    hipFunction_t f_rhs = nullptr, f_rk4_reg = nullptr, f_rk4_mem = nullptr, f_rk45_reg = nullptr,
                  f_rk45_mem = nullptr, f_multistep = nullptr, f_rk4_chain = nullptr, f_ros4 = nullptr, f_n1 = nullptr,
                  f_ros4_chain = nullptr, f_rk45_chain = nullptr, f_rk4_redo = nullptr, f_rk4_chain_redo = nullptr,
                  f_march = nullptr, f_campaign = nullptr, f_policy = nullptr, f_sens = nullptr, f_freq = nullptr;
    int n_cus = 0;
    DevBuf members;                          // the member rows [E][RMT_N2_MEMBER_FIXED + S + NU]
    // one status word per reactor + one word behind them: how many reactor-launches the cached RK4 steppers handed to
    // their plain twins so far (rmt_n2_fallbacks)
    // (a second word behind them: non-zero = rmt_n2_rk4_reg_redo integrates EVERY reactor, the cached stepper is skipped)
    DevBuf flags;
    DevBuf work;                             // stage arrays of the memory-resident steppers, in states [E][V][N]
    DevBuf mask;                             // one word per node of the one-workgroup stiff stepper
    DevBuf rings;                            // tagged-word links of the chained steppers: rings, decision slots, abort words
    DevBuf sync, slots;                      // chained RK4 stepper: 32 words and 8 (V + 1) doubles per link
    DevBuf backup, redo;                     // chained cached RK4 stepper: the launch's input, and its redo / status words
    DevBuf members1;                         // the rows of rmt_n1_profile
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // cached one-workgroup RK4 stepper: the fallback counter is copied back behind every cached launch (pinned word +
    // event, never waited for); when a launch lost at least half of its reactors to the plain stepper, the next
    // RMT_N2_PLAIN_LAUNCHES calls run the plain stepper alone
    unsigned* fb_host = nullptr;
    hipEvent_t ev_fb = nullptr;
    bool fb_pending = false;
    unsigned fb_seen = 0;
    int plain_left = 0;
    bool timed = false;
    int last_chunks = 1, last_teams = 0;     // geometry of the last stepper launch (rmt_n2_last_geometry)
    // axial profiles (code objects generated with RMT_PROFILE): the table [E][2][N] and the module's pointer to it
    int profiled = 0;
    DevBuf profile;
    hipDeviceptr_t profile_slot = nullptr;   // address of the module's `rmt_profile_tab`
    DevBuf law;                              // campaign units (RMT_CAMPAIGN): the deactivation law rows [E][5]
    // policy units (RMT_CAMPAIGN_POLICY): the rows [E][4] = {target, lo, hi, tolerance} with the carried coolant levels [E]
    // behind them in ONE allocation, and the index of the held component
    DevBuf policy;
    int policy_comp = -1;

    unsigned* status_words() const { return flags.as<unsigned>(); }
    // Runs on the handle's device (rmt_n2_destroy switches to it; rmt_n2_create has not left it); the buffers go after it.
    ~rmt_n2_handle() {
        if (fb_pending && ev_fb) (void)hipEventSynchronize(ev_fb);       // the counter copy into fb_host has landed
        if (ev_fb) (void)hipEventDestroy(ev_fb);
        if (fb_host) (void)hipHostFree(fb_host);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (module) (void)hipModuleUnload(module);
    }
};

// a profiled handle launches nothing before its table is there (the kernels would read through a null pointer)
static int profile_missing(const rmt_n2_handle* h) {
    if (h->profiled && !h->profile.p)
        return fail("this handle's code object was generated with RMT_PROFILE: call rmt_n2_set_profile before the "
                    "first launch");
    return 0;
}

// bytes of the member rows [E][RMT_N2_MEMBER_FIXED + S + NU], of one state [E][V][N] and of the profile table [E][2][N]
static size_t member_bytes(const rmt_n2_handle* h) { return (size_t)h->E * (RMT_N2_MEMBER_FIXED + h->S + h->NU) * sizeof(double); }
static size_t state_bytes(const rmt_n2_handle* h) { return (size_t)h->E * h->V * h->N * h->real_size; }
static size_t profile_bytes(const rmt_n2_handle* h) { return (size_t)h->E * 2 * (size_t)h->N * sizeof(double); }

// Every entry point runs on the device the handle was created on: workspace allocations, event
// records and module launches all act on the CURRENT device, which the caller may have changed
// since rmt_n2_create (multi-GPU hosts).  The guard switches to the handle's device and restores the
// caller's on scope exit.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    explicit DeviceGuard(const rmt_n2_handle* h) : DeviceGuard(h->device) {}
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define ON_DEVICE(h)                                                                        \
    DeviceGuard guard_(h);                                                                  \
    if (guard_.err != hipSuccess)                                                           \
        return fail("cannot switch to device %d of this handle: %s", (h)->device, hipGetErrorString(guard_.err))

extern "C" const char* rmt_n2_last_error(void) { return g_err.c_str(); }
extern "C" int rmt_n2_abi_version(void) { return RMT_N2_ABI_VERSION; }
extern "C" const char* rmt_n2_kernel_template(void) { return k_template; }
extern "C" const char* rmt_n2_hiprtc_path(void) {
    // the shared object hiprtcCompileProgram resolves to in THIS process
    Dl_info info;
    if (dladdr((void*)&hiprtcCompileProgram, &info) && info.dli_fname) return info.dli_fname;
    return "";
}
extern "C" void rmt_n2_free(void* p) { free(p); }
// Options every kernel is compiled with.  -disable-machine-licm: the machine-level loop-invariant code motion
// hoists the materialisation of fp64 literals (s_mov pairs) and compare masks out of the time-step loop into
// SGPRs, runs out of them and spills to VGPR lanes (v_writelane / v_readlane, full VALU slots) and, for the
// VGPR-resident ones, to scratch; without it the step loop of rmt_n2_rk45_reg has 2135 instead of 2294 VALU
// instructions and 4 instead of 13 scratch accesses (measured: +16 %; rmt_n2_rk4_reg +4 %, profiles/round2_issue_model.md).
static const char* const k_default_opts = "-O3 -std=c++17 -mllvm -disable-machine-licm";
extern "C" const char* rmt_n2_compile_options(void) { return k_default_opts; }

extern "C" int rmt_n2_compile(const char* source, const char* arch, const char* extra_opts,
                              void** code, size_t* code_size, char** log) {
    if (!source || !code || !code_size) return fail("rmt_n2_compile: null argument");
    *code = nullptr;
    *code_size = 0;
    if (log) *log = nullptr;
    hiprtcProgram prog;
    hiprtcResult r = hiprtcCreateProgram(&prog, source, "rmt_n2_generated.hip", 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) return fail("hiprtcCreateProgram: %s", hiprtcGetErrorString(r));
    std::string archopt = std::string("--offload-arch=") + (arch && *arch ? arch : "gfx950");
    std::vector<std::string> store = {archopt};
    // an -mllvm switch may be given only once: a caller that sets machine-licm itself replaces the default
    const bool own_licm = extra_opts && strstr(extra_opts, "machine-licm");
    for (std::string s : {std::string(own_licm ? "-O3 -std=c++17" : k_default_opts), std::string(extra_opts ? extra_opts : "")}) {
        size_t pos = 0;
        while (pos < s.size()) {
            size_t sp = s.find(' ', pos);
            if (sp == std::string::npos) sp = s.size();
            if (sp > pos) store.push_back(s.substr(pos, sp - pos));
            pos = sp + 1;
        }
    }
    std::vector<const char*> opts;
    for (auto& s : store) opts.push_back(s.c_str());
    r = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
    size_t logsz = 0;
    hiprtcGetProgramLogSize(prog, &logsz);
    std::string logs(logsz, '\0');
    if (logsz) hiprtcGetProgramLog(prog, &logs[0]);
    if (log && logsz) {
        *log = (char*)malloc(logsz + 1);
        memcpy(*log, logs.c_str(), logsz);
        (*log)[logsz] = 0;
    }
    if (r != HIPRTC_SUCCESS) {
        hiprtcDestroyProgram(&prog);
        return fail("hiprtcCompileProgram: %s\n%.1500s", hiprtcGetErrorString(r), logs.c_str());
    }
    size_t sz = 0;
    hiprtcGetCodeSize(prog, &sz);
    void* buf = malloc(sz);
    if (!buf) {
        hiprtcDestroyProgram(&prog);
        return fail("out of host memory for %zu byte code object", sz);
    }
    hiprtcGetCode(prog, (char*)buf);
    hiprtcDestroyProgram(&prog);
    *code = buf;
    *code_size = sz;
    return 0;
}

extern "C" int rmt_n2_create(const rmt_n2_plan* p, rmt_n2_handle** out) {
    if (!p || !out) return fail("rmt_n2_create: null argument");
    *out = nullptr;
    if (p->abi_version != RMT_N2_ABI_VERSION)
        return fail("ABI version mismatch: plan %d, library %d", p->abi_version, RMT_N2_ABI_VERSION);
    if (p->n_species < 1 || p->n_nodes < 2 || p->n_members < 1)
        return fail("bad plan sizes S=%d N=%d E=%d", p->n_species, p->n_nodes, p->n_members);
    if (p->n_vars != p->n_species && p->n_vars != p->n_species + 1)
        return fail("n_vars must be S or S+1 (got %d for S=%d)", p->n_vars, p->n_species);
    if (p->block < 64 || p->block > 1024 || p->block % 64)
        return fail("block must be a multiple of 64 in [64,1024] (got %d)", p->block);
    if (p->nodes_per_thread < 1) return fail("nodes_per_thread must be >= 1");
    if (p->n_user_params < 0 || p->n_user_params > 64) return fail("n_user_params must be in [0,64] (got %d)", p->n_user_params);
    if (p->ros4_nodes_per_block != 0 && p->ros4_nodes_per_block != p->block && p->ros4_nodes_per_block * 4 != p->block)
        return fail("ros4_nodes_per_block must be 0, block or block / 4 (got %d for block %d)", p->ros4_nodes_per_block, p->block);
    if (!p->code_object || !p->code_size || !p->members) return fail("plan lacks code object/members");
    if (p->profiled != 0 && p->profiled != 1) return fail("plan.profiled must be 0 or 1 (got %d)", p->profiled);
    if (p->profiled && p->fp32) return fail("profiled code objects (RMT_PROFILE) are fp64 only");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail("no HIP device available: the N2 integrator has no CPU fallback");
    std::unique_ptr<rmt_n2_handle> owner(new rmt_n2_handle());       // (every failing exit below releases what exists so far)
    rmt_n2_handle* h = owner.get();
    h->S = p->n_species;
    h->V = p->n_vars;
    h->NU = p->n_user_params;
    h->ros_nb = p->ros4_nodes_per_block > 0 ? p->ros4_nodes_per_block : p->block;
    h->N = p->n_nodes;
    h->E = p->n_members;
    h->fp32 = p->fp32;
    h->block = p->block;
    h->npt = p->nodes_per_thread;
    h->real_size = p->fp32 ? 4 : 8;
    h->profiled = p->profiled;
    HIP_OK(hipGetDevice(&h->device));
    HIP_OK(hipModuleLoadData(&h->module, p->code_object));
    // The kernels of the code object; the optional ones depend on what it was generated with.  rmt_n2_rk4_reg_redo /
    // rmt_n2_rk4_chain_redo: code objects whose RK4 stepper caches the temperature-only rate constants (RMT_KCACHE) carry
    // the plain stepper as a second kernel - it re-integrates the reactors the cached one gave up on.
    static const struct { const char* name; hipFunction_t rmt_n2_handle::*f; bool required; } kernels[] = {
        {"rmt_n2_rhs", &rmt_n2_handle::f_rhs, true},
        {"rmt_n2_rk4_reg", &rmt_n2_handle::f_rk4_reg, true},
        {"rmt_n2_rk4_mem", &rmt_n2_handle::f_rk4_mem, true},
        {"rmt_n2_rk4_reg_redo", &rmt_n2_handle::f_rk4_redo, false},
        {"rmt_n2_rk45_reg", &rmt_n2_handle::f_rk45_reg, false},
        {"rmt_n2_rk45_mem", &rmt_n2_handle::f_rk45_mem, false},
        {"rmt_n2_rk45_chain", &rmt_n2_handle::f_rk45_chain, false},
        {"rmt_n2_multistep_mem", &rmt_n2_handle::f_multistep, false},
        {"rmt_n2_rk4_chain", &rmt_n2_handle::f_rk4_chain, false},
        {"rmt_n2_rk4_chain_redo", &rmt_n2_handle::f_rk4_chain_redo, false},
        {"rmt_n2_ros4_mem", &rmt_n2_handle::f_ros4, false},
        {"rmt_n1_ros4", &rmt_n2_handle::f_n1, false},
        {"rmt_n2_ros4_chain", &rmt_n2_handle::f_ros4_chain, false},
        {"rmt_n2_steady_march", &rmt_n2_handle::f_march, false},
        {"rmt_n2_campaign_step", &rmt_n2_handle::f_campaign, false},
        {"rmt_n2_campaign_policy_step", &rmt_n2_handle::f_policy, false},
        {"rmt_n2_steady_sens", &rmt_n2_handle::f_sens, false},
        {"rmt_n2_steady_freq", &rmt_n2_handle::f_freq, false},
    };
    for (const auto& k : kernels) {
        const hipError_t e = hipModuleGetFunction(&(h->*k.f), h->module, k.name);
        if (e == hipSuccess) continue;
        h->*k.f = nullptr;
        if (k.required) return fail("hipModuleGetFunction(\"%s\") failed: %s", k.name, hipGetErrorString(e));
    }
    (void)hipGetLastError();
    if (h->profiled) {
        size_t bytes = 0;
        const hipError_t e = hipModuleGetGlobal(&h->profile_slot, &bytes, h->module, "rmt_profile_tab");
        if (e != hipSuccess || bytes != sizeof(double*))
            return fail("plan.profiled = 1, but the code object has no rmt_profile_tab (generate it with RMT_PROFILE 1): %s",
                        hipGetErrorString(e));
    }
    HIP_OK(hipDeviceGetAttribute(&h->n_cus, hipDeviceAttributeMultiprocessorCount, h->device));
    if (h->members.reserve(nullptr, member_bytes(h))) return 1;
    HIP_OK(hipMemcpy(h->members.p, p->members, member_bytes(h), hipMemcpyHostToDevice));
    if (h->flags.reserve(nullptr, ((size_t)h->E + 2) * sizeof(unsigned))) return 1;
    HIP_OK(hipMemset(h->flags.p, 0, h->flags.bytes));
    HIP_OK(hipHostMalloc((void**)&h->fb_host, 2 * sizeof(unsigned), hipHostMallocDefault));
    h->fb_host[0] = h->fb_host[1] = 0u;
    HIP_OK(hipEventCreateWithFlags(&h->ev_fb, hipEventDisableTiming));
    HIP_OK(hipEventCreate(&h->ev0));
    HIP_OK(hipEventCreate(&h->ev1));
    *out = owner.release();
    return 0;
}

extern "C" void rmt_n2_destroy(rmt_n2_handle* h) {
    if (!h) return;
    DeviceGuard guard_(h->device);
    delete h;
}

extern "C" int rmt_n2_set_stream(rmt_n2_handle* h, void* s) {
    if (!h) return fail("null handle");
    h->stream = (hipStream_t)s;
    return 0;
}

extern "C" int rmt_n2_set_mode(rmt_n2_handle* h, int mode) {
    if (!h) return fail("null handle");
    if (mode < 0 || mode > 3) return fail("mode must be 0 (auto), 1 (on-chip), 2 (memory) or 3 (chained)");
    h->mode = mode;
    return 0;
}

// new member rows, queued on the stream; `wait`: and the stream synchronised (the host array may be reused)
static int upload_members(rmt_n2_handle* h, const double* members, bool wait) {
    if (!h || !members) return fail("null argument");
    ON_DEVICE(h);
    HIP_OK(hipMemcpyAsync(h->members.p, members, member_bytes(h), hipMemcpyHostToDevice, h->stream));
    if (wait) HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int rmt_n2_set_members(rmt_n2_handle* h, const double* members) { return upload_members(h, members, true); }
extern "C" int rmt_n2_set_members_async(rmt_n2_handle* h, const double* members) { return upload_members(h, members, false); }

extern "C" int rmt_n2_get_members(rmt_n2_handle* h, double* members) {
    if (!h || !members) return fail("null argument");
    ON_DEVICE(h);
    HIP_OK(hipMemcpyAsync(members, h->members.p, member_bytes(h), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

// THE upload of a table the kernels read through the handle (profile, deactivation law, policy rows + levels): wait for
// the stream (a launch in flight may still read the old values), allocate on first use, then one blocking copy per part
// into the same buffer; with `slot` (the module's pointer to the table) that pointer is written and the device
// synchronised.  A handle whose FIRST upload failed keeps no buffer.
struct TablePart { const void* src; size_t bytes; };
static int upload_table(rmt_n2_handle* h, DevBuf* table, const char* who, std::initializer_list<TablePart> parts,
                        hipDeviceptr_t slot = nullptr) {
    size_t bytes = 0;
    for (const TablePart& part : parts) bytes += part.bytes;
    HIP_OK(hipStreamSynchronize(h->stream));
    const bool first = !table->p;
    if (table->reserve(h->stream, bytes)) return 1;
    hipError_t e = hipSuccess;
    size_t at = 0;
    for (const TablePart& part : parts) {
        if (e == hipSuccess) e = hipMemcpy(table->as<char>() + at, part.src, part.bytes, hipMemcpyHostToDevice);
        at += part.bytes;
    }
    if (e == hipSuccess && slot) e = hipMemcpyHtoD(slot, &table->p, sizeof table->p);
    if (e == hipSuccess && slot) e = hipDeviceSynchronize();
    if (e == hipSuccess) return 0;
    if (first) table->release();
    return fail("%s: %s", who, hipGetErrorString(e));
}

extern "C" int rmt_n2_set_profile(rmt_n2_handle* h, const double* table_host) {
    if (!h || !table_host) return fail("null argument");
    if (!h->profiled)
        return fail("rmt_n2_set_profile: this handle's code object was not generated with RMT_PROFILE (plan.profiled = 0)");
    ON_DEVICE(h);
    return upload_table(h, &h->profile, "rmt_n2_set_profile", {{table_host, profile_bytes(h)}}, h->profile_slot);
}

static int reserve_work(rmt_n2_handle* h, size_t arrays) { return h->work.reserve(h->stream, arrays * state_bytes(h)); }

// Reactors longer than one workgroup holds: C chunks of `width` nodes per reactor on C CUs, T teams, every workgroup
// resident (T*C <= #CUs).  ok: the device (and `limit`, the most chunks the kernel's links allow) admits that chain.
struct Chain { int C, T; bool ok; };
static Chain chain_geometry(const rmt_n2_handle* h, int width, int limit) {
    Chain g;
    g.C = (h->N + width - 1) / width;
    g.ok = g.C >= 2 && g.C <= h->n_cus && g.C <= limit;
    g.T = h->n_cus / g.C;
    if (g.T > h->E) g.T = h->E;
    return g;
}

// tagged-word links of the chained steppers: [links] rings of RMT_N2_RING entries of 2(V+1) words, then 2 decision
// words and one abort word per team; cleared before every launch (tag 0 never matches)
static int ensure_rings(rmt_n2_handle* h, const Chain& g, unsigned long long** decision, unsigned** abort_words) {
    const size_t words = 2 * (size_t)(h->V + 1);
    const size_t ring_words = (size_t)g.T * g.C * RMT_N2_RING * words;
    const size_t need = (ring_words + 2 * (size_t)g.T) * sizeof(unsigned long long) + (size_t)g.T * sizeof(unsigned);
    if (h->rings.reserve(h->stream, need)) return 1;
    HIP_OK(hipMemsetAsync(h->rings.p, 0, need, h->stream));
    *decision = h->rings.as<unsigned long long>() + ring_words;
    *abort_words = (unsigned*)(*decision + 2 * (size_t)g.T);
    return 0;
}

// THE kernel launch: function, grid, block and arguments
static int launch(hipStream_t stream, hipFunction_t f, size_t grid, int block, void** args) {
    HIP_OK(hipModuleLaunchKernel(f, (unsigned)grid, 1, 1, (unsigned)block, 1, 1, 0, stream, args, nullptr));
    return 0;
}

// THE timed bracket of a handle (rmt_n2_last_kernel_ms): ev0, whatever `launches` queues, ev1
template <class Launches>
static int timed_region(rmt_n2_handle* h, Launches launches) {
    HIP_OK(hipEventRecord(h->ev0, h->stream));
    if (launches()) return 1;
    HIP_OK(hipEventRecord(h->ev1, h->stream));
    h->timed = true;
    return 0;
}

// The launch of a stepper (or of the RHS kernel) at the handle's block size, timed and noted for rmt_n2_last_geometry:
// `teams` teams of `chunks` workgroups each - 0 teams: one workgroup per reactor, or `grid` of them walking the reactors.
// Several kernels: one behind the other with the same arguments and geometry, inside one bracket.
static int launch_stepper(rmt_n2_handle* h, std::initializer_list<hipFunction_t> kernels, void** args, int chunks = 1,
                          int teams = 0, size_t grid = 0) {
    h->last_chunks = chunks;
    h->last_teams = teams > 0 ? teams : h->E;
    if (!grid) grid = teams > 0 ? (size_t)teams * chunks : (size_t)h->E;
    return timed_region(h, [&]() -> int {
        for (hipFunction_t f : kernels)
            if (launch(h->stream, f, grid, h->block, args)) return 1;
        return 0;
    });
}

// one lane per reactor (or per `lanes` of another count), one wave per workgroup: the N1 kernel and the per-lane marches
// (kernels/71 .. 74); the stepper geometry stays what it was
static int launch_lanes(rmt_n2_handle* h, hipFunction_t f, void** args, size_t lanes = 0) {
    return timed_region(h, [&] { return launch(h->stream, f, ((lanes ? lanes : (size_t)h->E) + 63) / 64, 64, args); });
}

extern "C" int rmt_n2_last_geometry(rmt_n2_handle* h, int* chunks, int* teams) {
    if (!h || !chunks || !teams) return fail("null argument");
    *chunks = h->last_chunks;
    *teams = h->last_teams;
    return 0;
}

extern "C" int rmt_n2_last_kernel_ms(rmt_n2_handle* h, float* ms) {
    if (!h || !ms) return fail("null argument");
    if (!h->timed) return fail("no launch recorded yet");
    ON_DEVICE(h);
    HIP_OK(hipEventSynchronize(h->ev1));
    HIP_OK(hipEventElapsedTime(ms, h->ev0, h->ev1));
    return 0;
}

extern "C" int rmt_n2_rhs(rmt_n2_handle* h, double t, const void* y, void* dydt) {
    (void)t; /* the N2 right-hand side is autonomous (pbHomoReactor.py:3706: t unused) */
    if (!h || !y || !dydt) return fail("null argument");
    if (profile_missing(h)) return 1;
    ON_DEVICE(h);
    int N = h->N, E = h->E;
    void* args[] = {(void*)&y, (void*)&dydt, (void*)&h->members.p, (void*)&N, (void*)&E, (void*)&h->flags.p};
    // persistent workgroups: at most RMT_N2_RHS_WGS_PER_CU per CU, each walking reactors e, e + grid, ...
    static const int per_cu = [] {               // tuning override, read once
        const char* v = getenv("RMT_N2_RHS_WGS_PER_CU");
        const int n = v ? atoi(v) : 0;
        return n > 0 ? n : RMT_N2_RHS_WGS_PER_CU;
    }();
    const long long cap = (long long)h->n_cus * per_cu;
    return launch_stepper(h, {h->f_rhs}, args, 1, 0, h->E < cap ? (size_t)h->E : (size_t)cap);
}

static bool fits_registers(const rmt_n2_handle* h) { return h->N <= h->block * h->npt; }

// Caching RK4 steppers: did the last cached launch lose at least half of its reactors to the plain stepper (a transient
// faster than the cache's range serves)?  Then the cached pass would only be run in vain for a while: true = this call
// runs the plain stepper alone.  The counter behind the status words is copied back behind every cached launch (pinned
// word + event, never waited for).
static bool plain_this_call(rmt_n2_handle* h) {
    if (h->fb_pending && hipEventQuery(h->ev_fb) == hipSuccess) {
        h->fb_pending = false;
        const unsigned lost = h->fb_host[0] - h->fb_seen;
        h->fb_seen = h->fb_host[0];
        if (2u * lost >= (unsigned)h->E) h->plain_left = RMT_N2_PLAIN_LAUNCHES;
    }
    if (h->plain_left <= 0) return false;
    --h->plain_left;
    return true;
}

static int copy_back_fallbacks(rmt_n2_handle* h) {
    if (h->fb_pending) return 0;
    HIP_OK(hipMemcpyAsync(h->fb_host, h->status_words() + h->E, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipEventRecord(h->ev_fb, h->stream));
    h->fb_pending = true;
    return 0;
}

static bool capturing(rmt_n2_handle* h) {      // (the policy reads an event and copies to host memory: not under capture)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return h->stream && hipStreamIsCapturing(h->stream, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

extern "C" int rmt_n2_rk4(rmt_n2_handle* h, void* y, double t0, double dt, int64_t nsteps) {
    (void)t0;
    if (!h || !y) return fail("null argument");
    if (!(dt > 0) || nsteps < 0) return fail("rk4 needs dt > 0 and nsteps >= 0");
    if (profile_missing(h)) return 1;
    ON_DEVICE(h);
    int N = h->N, E = h->E;
    long long ns = (long long)nsteps;
    const bool reg = h->mode == 1 || (h->mode == 0 && fits_registers(h));
    if (reg) {
        if (!fits_registers(h))
            return fail("register-resident stepper holds at most %d nodes per reactor (N=%d)",
                        h->block * h->npt, h->N);
        void* args[] = {(void*)&y, (void*)&h->members.p, (void*)&N, (void*)&dt, (void*)&ns,
                        (void*)&h->flags.p};
        if (!h->f_rk4_redo) return launch_stepper(h, {h->f_rk4_reg}, args);
        // (a stream that is being captured into a graph gets the two kernels and nothing else)
        if (capturing(h)) {
            if (launch(h->stream, h->f_rk4_reg, h->E, h->block, args)) return 1;
            return launch(h->stream, h->f_rk4_redo, h->E, h->block, args);
        }
        if (plain_this_call(h)) {        // flags[E + 1] != 0: rmt_n2_rk4_reg_redo integrates every reactor
            HIP_OK(hipMemsetAsync(h->status_words() + h->E + 1, 1, sizeof(unsigned), h->stream));
            const int rc = launch_stepper(h, {h->f_rk4_redo}, args);
            HIP_OK(hipMemsetAsync(h->status_words() + h->E + 1, 0, sizeof(unsigned), h->stream));
            return rc;
        }
        // the cached stepper, and behind it the plain one for the reactors it gave up on
        if (launch_stepper(h, {h->f_rk4_reg, h->f_rk4_redo}, args)) return 1;
        return copy_back_fallbacks(h);
    }
    const Chain g = chain_geometry(h, h->block * h->npt, h->n_cus);
    const bool can_chain = h->f_rk4_chain && g.ok;
    if (h->mode == 3 && !can_chain)
        return fail("chained stepper needs 2 <= chunks (%d) <= CUs (%d)", g.C, h->n_cus);
    if (h->mode == 3 || (h->mode == 0 && can_chain)) {
        int C = g.C, T = g.T;
        const size_t links = (size_t)T * C, sync_bytes = links * 32 * sizeof(unsigned long long);
        if (h->sync.reserve(h->stream, sync_bytes)) return 1;
        if (h->slots.reserve(h->stream, links * 8 * (size_t)(h->V + 1) * sizeof(double))) return 1;
        // a chained stepper that caches the temperature-only rate constants (RMT_KCACHE_CHAIN) saves the launch's input
        // and is followed by rmt_n2_rk4_chain_redo on the same grid, see kernels/50_rk4.inc rmt_rk4_chain_body
        void* backup = nullptr;
        unsigned *redo = nullptr, *falt = nullptr;
        if (h->f_rk4_chain_redo) {
            const size_t redo_bytes = 2 * (size_t)h->E * sizeof(unsigned);
            if (h->backup.reserve(h->stream, state_bytes(h)) || h->redo.reserve(h->stream, redo_bytes)) return 1;
            backup = h->backup.p;
            redo = h->redo.as<unsigned>();
            falt = redo + h->E;
            HIP_OK(hipMemsetAsync(redo, 0, redo_bytes, h->stream));
        }
        // the same policy as for the one-workgroup stepper: after a launch that lost half of its reactors the plain
        // chained stepper runs alone for a while - every redo word set (to a value the fallback counter does not count),
        // the input copied to the backup buffer the plain stepper reads
        const bool plain = h->f_rk4_chain_redo && !capturing(h) && plain_this_call(h);
        if (plain) {
            HIP_OK(hipMemcpyAsync(backup, y, state_bytes(h), hipMemcpyDeviceToDevice, h->stream));
            HIP_OK(hipMemsetAsync(redo, 2, (size_t)h->E * sizeof(unsigned), h->stream));
        }
        unsigned long long* decision = nullptr;
        unsigned* abort_words = nullptr;
        void* args[] = {(void*)&y, (void*)&h->members.p, (void*)&N, (void*)&E, (void*)&C, (void*)&T,
                        (void*)&dt, (void*)&ns, (void*)&h->sync.p, (void*)&h->slots.p, (void*)&h->flags.p,
                        (void*)&h->rings.p, (void*)&abort_words, (void*)&backup, (void*)&redo, (void*)&falt};
        h->last_chunks = C;
        h->last_teams = T;
        const int rc = timed_region(h, [&]() -> int {
            for (hipFunction_t f : {plain ? (hipFunction_t) nullptr : h->f_rk4_chain, h->f_rk4_chain_redo}) {
                if (!f) continue;
                HIP_OK(hipMemsetAsync(h->sync.p, 0, sync_bytes, h->stream));
                if (ensure_rings(h, g, &decision, &abort_words)) return 1;
                if (launch(h->stream, f, links, h->block, args)) return 1;
            }
            return 0;
        });
        if (rc) return rc;
        if (h->f_rk4_chain_redo && !plain && !capturing(h)) return copy_back_fallbacks(h);
        return 0;
    }
    if (reserve_work(h, 3)) return 1;
    void* args[] = {(void*)&y, (void*)&h->work.p, (void*)&h->members.p, (void*)&N, (void*)&E,
                    (void*)&dt, (void*)&ns, (void*)&h->flags.p};
    return launch_stepper(h, {h->f_rk4_mem}, args);
}

extern "C" int rmt_n2_multistep(rmt_n2_handle* h, void* y, double t0, double dt, int64_t nsteps,
                                int method) {
    (void)t0;
    if (!h || !y) return fail("null argument");
    if (!(dt > 0) || nsteps < 3) return fail("multistep needs dt > 0 and nsteps >= 3");
    if (method != 0 && method != 1) return fail("method must be 0 (AdBash3) or 1 (PreCorr3)");
    if (!h->f_multistep) return fail("code object has no multistep kernel");
    if (profile_missing(h)) return 1;
    ON_DEVICE(h);
    if (reserve_work(h, 8)) return 1;
    int N = h->N, E = h->E;
    long long ns = (long long)nsteps;
    void* args[] = {(void*)&y, (void*)&h->work.p, (void*)&h->members.p, (void*)&N, (void*)&E,
                    (void*)&dt, (void*)&ns, (void*)&method, (void*)&h->flags.p};
    return launch_stepper(h, {h->f_multistep}, args);
}

extern "C" int rmt_n2_rk45(rmt_n2_handle* h, void* y, double t0, double t1, double rtol, double atol,
                           double h0, int64_t max_steps, rmt_n2_stats* stats) {
    if (!h || !y || !stats) return fail("null argument");
    if (!(t1 > t0) || !(rtol > 0) || !(atol >= 0) || !(h0 != 0)) return fail("bad rk45 arguments");
    if (profile_missing(h)) return 1;
    ON_DEVICE(h);
    int N = h->N, E = h->E;
    long long ms = (long long)max_steps;
    const bool reg = (h->mode == 1 || (h->mode == 0 && fits_registers(h))) && h->f_rk45_reg;
    if (reg) {
        if (!fits_registers(h)) return fail("register-resident rk45 does not fit N=%d", h->N);
        void* args[] = {(void*)&y, (void*)&h->members.p, (void*)&N, (void*)&t0, (void*)&t1,
                        (void*)&rtol, (void*)&atol, (void*)&h0, (void*)&ms, (void*)&stats,
                        (void*)&h->flags.p};
        return launch_stepper(h, {h->f_rk45_reg}, args);
    }
    // Reactors longer than one workgroup's on-chip capacity: rmt_n2_rk45_chain (the code object has it when the on-chip
    // slots fit the geometry).
    const Chain g = chain_geometry(h, h->block * h->npt, RMT_N2_MAX_CHUNKS);
    const bool can_chain = h->f_rk45_chain && g.ok;
    if (h->mode == 3 && !can_chain)
        return fail("chained rk45 needs the on-chip stepper in the code object and 2 <= chunks (%d) <= %d", g.C,
                    h->n_cus < RMT_N2_MAX_CHUNKS ? h->n_cus : RMT_N2_MAX_CHUNKS);
    if (can_chain && (h->mode == 3 || h->mode == 0)) {
        int C = g.C, T = g.T;
        unsigned long long* decision = nullptr;
        unsigned* abort_words = nullptr;
        if (ensure_rings(h, g, &decision, &abort_words)) return 1;
        void* args[] = {(void*)&y, (void*)&h->members.p, (void*)&N, (void*)&E, (void*)&C, (void*)&T, (void*)&t0,
                        (void*)&t1, (void*)&rtol, (void*)&atol, (void*)&h0, (void*)&ms, (void*)&stats,
                        (void*)&h->flags.p, (void*)&h->rings.p, (void*)&decision, (void*)&abort_words};
        return launch_stepper(h, {h->f_rk45_chain}, args, C, T);
    }
    if (!h->f_rk45_mem) return fail("code object has no rk45 kernel");
    if (reserve_work(h, 10)) return 1;     // K_1..K_7 (when they do not fit in LDS), y_new, K_1/K_7 of the FSAL swap
    void* args[] = {(void*)&y, (void*)&h->work.p, (void*)&h->members.p, (void*)&N, (void*)&E,
                    (void*)&t0, (void*)&t1, (void*)&rtol, (void*)&atol, (void*)&h0, (void*)&ms,
                    (void*)&stats, (void*)&h->flags.p};
    return launch_stepper(h, {h->f_rk45_mem}, args);
}

extern "C" int rmt_n2_ros4(rmt_n2_handle* h, void* y, double t0, double t1, double rtol, double atol,
                           double h0, int64_t max_steps, rmt_n2_stats* stats) {
    if (!h || !y || !stats) return fail("null argument");
    if (!(t1 > t0) || !(rtol > 0) || !(atol >= 0) || !(h0 != 0)) return fail("bad ros4 arguments");
    if (!h->f_ros4) return fail("code object has no ros4 kernel");
    if (profile_missing(h)) return 1;
    ON_DEVICE(h);
    if (h->block > 512)
        return fail("the Rosenbrock kernel holds a VxV matrix per lane: generate the code object with "
                    "block <= 512 (got %d)", h->block);
    // One reactor over several CUs (rmt_n2_ros4_chain): C chunks of W nodes per reactor, T teams, every
    // workgroup resident (T*C <= #CUs).  Auto mode chains when the ensemble alone cannot fill the device.
    const int nblocks = (h->N + h->ros_nb - 1) / h->ros_nb;      // node blocks per reactor
    int C = 1;
    if (h->f_ros4_chain && h->npt == 1 && nblocks >= 2 && h->mode != 2) {
        // Chunks of ONE node block pipeline stage by stage (a chunk lags its upstream neighbour by a message
        // latency, ~0.3 stage-block times); chunks of b > 1 blocks run all six stages of a block before the
        // next one (the block's stage vectors live in LDS), so a downstream chunk starts 6(b-1) stage-block
        // times late.  Estimated step time in stage-block units, minimised over the chunk count:
        // The T = #CUs / C teams of a launch work through the reactors in rounds of T, so the job costs
        // ceil(E / T) rounds of that step time - against ceil(E / #CUs) rounds of 6 nblocks for one workgroup per
        // reactor.  (Few chunks of several blocks lose to many one-block chunks run in more rounds: 8 reactors of
        // 16384 nodes take 2.99 s as 32 chunks x 8 teams and 0.36 s as 64 chunks x 4 teams x 2 rounds.)
        int cmax = nblocks < h->n_cus ? nblocks : h->n_cus;
        if (cmax > RMT_N2_MAX_CHUNKS) cmax = RMT_N2_MAX_CHUNKS;
        double best = 6.0 * nblocks * ((h->E + h->n_cus - 1) / h->n_cus);
        for (int c = 2; c <= cmax; ++c) {
            const int b = (nblocks + c - 1) / c;
            const int cc = (nblocks + b - 1) / b;
            int teams = h->n_cus / cc;
            if (teams > h->E) teams = h->E;
            const int rounds = (h->E + teams - 1) / teams;
            // (x 1.35: a chained stage-block is slower than a resident one - its sweeps exchange the chunk
            // boundary over the links; calibrated on the 4096-node reactor, 97 us per step in 16 chunks)
            const double cost = 1.35 * rounds * (6.0 * b + (cc - 1) * (6.0 * (b - 1) + 0.3));
            if (cost < best || (h->mode == 3 && C < 2)) { best = cost; C = cc; }
        }
        if (const char* force = getenv("RMT_N2_ROS4_CHUNKS")) {       // tuning experiments: chunk count by hand
            const int c = atoi(force);
            if (c >= 1 && c <= cmax) C = c;
        }
    }
    if (h->mode == 3 && C < 2)
        return fail("chained stiff stepper needs >= 2 node blocks per reactor (N=%d block=%d E=%d CUs=%d)",
                    h->N, h->block, h->E, h->n_cus);
    int N = h->N, E = h->E;
    long long ms = (long long)max_steps;
    if (C >= 2) {
        int W = (nblocks + C - 1) / C * h->ros_nb;      // whole node blocks per chunk; the chunks that many nodes make
        const Chain g = chain_geometry(h, W, RMT_N2_MAX_CHUNKS);
        int T = g.T;
        C = g.C;
        if (reserve_work(h, 1)) return 1;               // y_new
        unsigned long long* decision = nullptr;
        unsigned* abort_words = nullptr;
        if (ensure_rings(h, g, &decision, &abort_words)) return 1;
        void* args[] = {(void*)&y, (void*)&h->work.p, (void*)&h->members.p, (void*)&N, (void*)&E, (void*)&C, (void*)&T,
                        (void*)&W, (void*)&t0, (void*)&t1, (void*)&rtol, (void*)&atol, (void*)&h0, (void*)&ms,
                        (void*)&stats, (void*)&h->flags.p, (void*)&h->rings.p, (void*)&decision, (void*)&abort_words};
        return launch_stepper(h, {h->f_ros4_chain}, args, C, T);
    }
    // 7 vector arrays + the VxV inverse per node (= V more "vector arrays")
    if (reserve_work(h, 8 + (size_t)h->V)) return 1;   // 7 stage arrays + VxV inverses + upwind coupling (model M2)
    if (h->mask.reserve(h->stream, (size_t)h->E * h->N * sizeof(unsigned))) return 1;
    void* args[] = {(void*)&y, (void*)&h->work.p, (void*)&h->mask.p, (void*)&h->members.p, (void*)&N,
                    (void*)&E, (void*)&t0, (void*)&t1, (void*)&rtol, (void*)&atol, (void*)&h0,
                    (void*)&ms, (void*)&stats, (void*)&h->flags.p};
    return launch_stepper(h, {h->f_ros4}, args);
}

extern "C" int rmt_n1_profile(rmt_n2_handle* h, const double* members1, void* out, int nout, double rtol,
                              double atol, double h0, int64_t max_steps, rmt_n2_stats* stats) {
    if (!h || !members1 || !out || !stats) return fail("null argument");
    if (nout < 2 || !(rtol > 0) || !(atol >= 0) || !(h0 > 0)) return fail("bad N1 arguments");
    if (!h->f_n1) return fail("code object has no N1 kernel");
    if (profile_missing(h)) return 1;
    ON_DEVICE(h);
    if (h->members1.reserve(h->stream, member_bytes(h))) return 1;
    HIP_OK(hipMemcpyAsync(h->members1.p, members1, member_bytes(h), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    int E = h->E;
    long long ms = (long long)max_steps;
    void* args[] = {(void*)&h->members1.p, (void*)&out, (void*)&E, (void*)&nout, (void*)&rtol, (void*)&atol,
                    (void*)&h0, (void*)&ms, (void*)&stats, (void*)&h->flags.p};
    return launch_lanes(h, h->f_n1, args);
}

extern "C" int rmt_n2_steady_march(rmt_n2_handle* h, void* y_out, double tol, int64_t max_iter, rmt_n2_stats* stats) {
    if (!h || !y_out || !stats) return fail("null argument");
    if (!(tol > 0) || max_iter < 1) return fail("bad steady-march arguments (tolerance > 0, max_iter >= 1)");
    if (!h->f_march) return fail("code object has no rmt_n2_steady_march (generate it with RMT_WITH_MARCH)");
    if (h->fp32) return fail("the steady-state march is fp64 only");
    if (profile_missing(h)) return 1;
    ON_DEVICE(h);
    int N = h->N, E = h->E;
    long long mi = (long long)max_iter;
    void* args[] = {(void*)&y_out, (void*)&h->members.p, (void*)&N, (void*)&E, (void*)&tol, (void*)&mi, (void*)&stats,
                    (void*)&h->flags.p};
    return launch_lanes(h, h->f_march, args);
}

// The descriptor of the sensitivity and the frequency sweep travels by value: {kind[8], index[8]} as the kernels declare
// it.  ``who``: the entry point, ``what``: "parameter" / "input" (for the error text); kinds 0 TM, 1 THETA_IN, 2 P0,
// 3 CIN[index] and - where ``max_kind`` is 4 - 4 user column [index].
#define RMT_N2_SENS_MAX 8
struct ParamDesc { int kind[RMT_N2_SENS_MAX], index[RMT_N2_SENS_MAX]; };
static int build_desc(const rmt_n2_handle* h, const char* who, const char* what, int max_kind, int n, const int* kinds,
                      const int* indices, ParamDesc* desc) {
    std::memset(desc, 0, sizeof(*desc));
    const bool user = max_kind >= 4;
    for (int p = 0; p < n; ++p) {
        const int k = kinds[p], i = indices[p];
        if (k < 0 || k > max_kind || i < 0 || (k == 3 && i >= h->S) || (k == 4 && i >= h->NU) || (k < 3 && i != 0))
            return fail("%s: %s %d: kind %d (0 TM, 1 THETA_IN, 2 P0, 3 CIN[index]%s) with index %d is out of range (S = %d%s)",
                        who, what, p, k, user ? ", 4 user column [index]" : "", i, h->S,
                        user ? (", NU = " + std::to_string(h->NU)).c_str() : "");
        desc->kind[p] = k;
        desc->index[p] = i;
    }
    return 0;
}

// solver-config "sensitivity" (kernels/73_sensitivity.inc): the tangent march over the converged state, behind
// rmt_n2_steady_march on the same handle.
extern "C" int rmt_n2_steady_sens(rmt_n2_handle* h, const void* y, int n_params, const int* kinds, const int* indices,
                                  double* out) {
    if (!h || !y || !kinds || !indices || !out) return fail("rmt_n2_steady_sens: null argument");
    if (!h->f_sens || !h->f_march)
        return fail("rmt_n2_steady_sens: this handle's code object has no rmt_n2_steady_sens (generate it with RMT_SENS and "
                    "RMT_SENS_NP beside RMT_WITH_MARCH)");
    if (h->fp32) return fail("rmt_n2_steady_sens: fp64 only");
    if (n_params < 1 || n_params > RMT_N2_SENS_MAX) return fail("rmt_n2_steady_sens: 1..8 parameters (got %d)", n_params);
    ParamDesc desc;
    if (build_desc(h, "rmt_n2_steady_sens", "parameter", 4, n_params, kinds, indices, &desc)) return 1;
    if (profile_missing(h)) return 1;
    ON_DEVICE(h);
    int N = h->N, E = h->E;
    void* args[] = {(void*)&y, (void*)&h->members.p, (void*)&N, (void*)&E, (void*)&n_params, (void*)&desc, (void*)&out,
                    (void*)&h->flags.p};
    return launch_lanes(h, h->f_sens, args);
}

// solver-config "frequency-response" (kernels/74_frequency.inc): the shifted tangent march over the converged state, one
// (member, frequency) pair per lane.  Frequencies and peak nodes are HOST arrays, the result comes back to the HOST: the
// call uploads, launches once, copies back and synchronises; its device buffer lives for the call.
#define RMT_N2_FREQ_MAX_INPUTS 4
#define RMT_N2_FREQ_MAX_FREQUENCIES 4096
extern "C" int rmt_n2_steady_freq(rmt_n2_handle* h, const void* y, int n_inputs, const int* kinds, const int* indices,
                                  int n_freq, const double* omegas_host, const int* peak_nodes_host, int profile,
                                  double* out_host) {
    if (!h || !y || !kinds || !indices || !omegas_host || !peak_nodes_host || !out_host)
        return fail("rmt_n2_steady_freq: null argument");
    if (!h->f_freq || !h->f_march)
        return fail("rmt_n2_steady_freq: this handle's code object has no rmt_n2_steady_freq (generate it with RMT_FREQ and "
                    "RMT_FREQ_NP beside RMT_SENS and RMT_WITH_MARCH)");
    if (h->fp32) return fail("rmt_n2_steady_freq: fp64 only");
    if (n_inputs < 1 || n_inputs > RMT_N2_FREQ_MAX_INPUTS)
        return fail("rmt_n2_steady_freq: 1..%d inputs (got %d)", RMT_N2_FREQ_MAX_INPUTS, n_inputs);
    if (n_freq < 1 || n_freq > RMT_N2_FREQ_MAX_FREQUENCIES)
        return fail("rmt_n2_steady_freq: 1..%d frequencies (got %d)", RMT_N2_FREQ_MAX_FREQUENCIES, n_freq);
    ParamDesc desc;
    if (build_desc(h, "rmt_n2_steady_freq", "input", 3, n_inputs, kinds, indices, &desc)) return 1;
    for (int f = 0; f < n_freq; ++f)
        if (!(omegas_host[f] >= 0.0) || !std::isfinite(omegas_host[f]))
            return fail("rmt_n2_steady_freq: frequency %d is %g (finite and >= 0)", f, omegas_host[f]);
    if (profile_missing(h)) return 1;
    ON_DEVICE(h);
    const size_t lanes = (size_t)h->E * (size_t)n_freq, rows = (size_t)n_inputs * (size_t)(h->V + 1) * 2;
    const size_t n_out = lanes * rows * 2, n_tab = profile ? lanes * rows * (size_t)h->N : 0, n_all = n_out + n_tab + lanes;
    const size_t omega_bytes = (size_t)n_freq * sizeof(double), peak_bytes = (size_t)h->E * sizeof(int);
    if ((lanes + 63) / 64 > 0x7fffffffULL) return fail("rmt_n2_steady_freq: %zu lanes are more than one grid holds", lanes);
    DevBuf buf;                                                   // (freed on every way out)
    if (buf.reserve(h->stream, n_all * sizeof(double) + omega_bytes + peak_bytes)) return 1;
    double* d_out = buf.as<double>();
    double* d_tab = profile ? d_out + n_out : nullptr;
    double* d_failed = d_out + n_out + n_tab;
    double* d_omegas = d_out + n_all;
    int* d_peak = (int*)(d_omegas + n_freq);
    HIP_OK(hipMemsetAsync(d_out, 0, n_all * sizeof(double), h->stream));
    HIP_OK(hipMemcpyAsync(d_omegas, omegas_host, omega_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipMemcpyAsync(d_peak, peak_nodes_host, peak_bytes, hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));                      // (the host arrays are pageable: the copies have left them)
    int N = h->N, E = h->E;
    void* args[] = {(void*)&y, (void*)&h->members.p, (void*)&N, (void*)&E, (void*)&n_freq, (void*)&n_inputs, (void*)&desc,
                    (void*)&d_omegas, (void*)&d_peak, (void*)&profile, (void*)&d_out, (void*)&d_tab, (void*)&d_failed,
                    (void*)&h->flags.p};
    if (launch_lanes(h, h->f_freq, args, lanes)) return 1;
    HIP_OK(hipMemcpyAsync(out_host, d_out, n_all * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------- campaign
// solver-config "deactivation" (kernels/72_campaign.inc).  Each of the three entry points needs a code object with
// rmt_n2_campaign_step, a profile table (rmt_n2_set_profile) and a law (rmt_n2_set_campaign_law); the first one sets the law
// and therefore checks only what comes before it.
#define RMT_N2_CAMPAIGN_LAW 5
static int campaign_ready(const rmt_n2_handle* h, const char* who, bool need_law) {
    if (!h->f_campaign)
        return fail("%s: this handle's code object has no rmt_n2_campaign_step (generate it with RMT_CAMPAIGN, "
                    "RMT_WITH_MARCH and RMT_PROFILE)", who);
    if (!h->profiled || !h->profile.p) return fail("%s: no profile table has been set (rmt_n2_set_profile comes first)", who);
    if (need_law && !h->law.p) return fail("%s: no deactivation law has been set (rmt_n2_set_campaign_law comes first)", who);
    return 0;
}

extern "C" int rmt_n2_set_campaign_law(rmt_n2_handle* h, const double* law_host) {
    if (!h || !law_host) return fail("rmt_n2_set_campaign_law: null argument");
    if (campaign_ready(h, "rmt_n2_set_campaign_law", false)) return 1;
    for (int e = 0; e < h->E; ++e) {
        const double* l = law_host + (size_t)e * RMT_N2_CAMPAIGN_LAW;
        if (!(l[0] > 0) || !(l[1] >= 0) || !(l[2] > 0) || !(l[3] >= 1) || !(l[4] >= 0 && l[4] < 1) || std::isinf(l[0]) ||
            std::isinf(l[1]) || std::isinf(l[2]) || std::isinf(l[3]))
            return fail("rmt_n2_set_campaign_law: member %d: need k_ref > 0, Ed >= 0, Tref > 0, m >= 1, 0 <= a_inf < 1, all "
                        "finite", e);
    }
    ON_DEVICE(h);
    return upload_table(h, &h->law, "rmt_n2_set_campaign_law", {{law_host, (size_t)h->E * RMT_N2_CAMPAIGN_LAW * sizeof(double)}});
}

extern "C" int rmt_n2_campaign_step(rmt_n2_handle* h, void* y, double dt, double tol, int64_t max_iter, double* log_row,
                                    rmt_n2_stats* stats) {
    if (!h || !y || !log_row || !stats) return fail("rmt_n2_campaign_step: null argument");
    if (campaign_ready(h, "rmt_n2_campaign_step", true)) return 1;
    if (!(tol > 0) || max_iter < 1 || !(dt >= 0) || std::isinf(dt))
        return fail("rmt_n2_campaign_step: bad arguments (dt >= 0 and finite, tolerance > 0, max_iter >= 1)");
    if (h->fp32) return fail("rmt_n2_campaign_step: fp64 only");
    ON_DEVICE(h);
    int N = h->N, E = h->E;
    long long mi = (long long)max_iter;
    void* args[] = {(void*)&y, (void*)&h->members.p, (void*)&N, (void*)&E, (void*)&tol, (void*)&mi, (void*)&stats,
                    (void*)&h->flags.p, (void*)&h->profile.p, (void*)&h->law.p, (void*)&dt, (void*)&log_row};
    return launch_lanes(h, h->f_campaign, args);
}

extern "C" int rmt_n2_get_profile(rmt_n2_handle* h, double* table_host) {
    if (!h || !table_host) return fail("rmt_n2_get_profile: null argument");
    if (campaign_ready(h, "rmt_n2_get_profile", true)) return 1;
    ON_DEVICE(h);
    HIP_OK(hipMemcpyAsync(table_host, h->profile.p, profile_bytes(h), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

// The coolant policy of a campaign (solver-config "deactivation" "policy", kernels/72_campaign.inc under
// RMT_CAMPAIGN_POLICY).  Each of the three entry points needs what the campaign's need and a code object with
// rmt_n2_campaign_policy_step; the second and third also the policy rows, which the first one sets.
#define RMT_N2_POLICY_ROW 4
static int policy_ready(const rmt_n2_handle* h, const char* who, bool need_policy) {
    if (!h->f_policy)
        return fail("%s: this handle's code object has no rmt_n2_campaign_policy_step (generate it with RMT_CAMPAIGN_POLICY "
                    "beside RMT_CAMPAIGN, RMT_WITH_MARCH and RMT_PROFILE)", who);
    if (campaign_ready(h, who, true)) return 1;
    if (need_policy && !h->policy.p)
        return fail("%s: no policy has been set (rmt_n2_set_campaign_policy comes first)", who);
    return 0;
}
// the carried coolant levels [E] behind the policy rows [E][RMT_N2_POLICY_ROW]
static double* policy_levels(const rmt_n2_handle* h) { return h->policy.as<double>() + (size_t)h->E * RMT_N2_POLICY_ROW; }

extern "C" int rmt_n2_set_campaign_policy(rmt_n2_handle* h, const double* rows_host, int component,
                                          const double* levels_host) {
    if (!h || !rows_host || !levels_host) return fail("rmt_n2_set_campaign_policy: null argument");
    if (policy_ready(h, "rmt_n2_set_campaign_policy", false)) return 1;
    if (component < 0 || component >= h->S)
        return fail("rmt_n2_set_campaign_policy: bad arguments (component %d is not one of the %d species)", component, h->S);
    for (int e = 0; e < h->E; ++e) {
        const double* r = rows_host + (size_t)e * RMT_N2_POLICY_ROW;
        const double l = levels_host[e];
        if (!(r[0] > 0 && r[0] < 1) || !(r[1] > 0) || !(r[1] <= r[2]) || std::isinf(r[2]) || !(r[3] > 0) || std::isinf(r[3]) ||
            !(l >= r[1] && l <= r[2]))
            return fail("rmt_n2_set_campaign_policy: bad arguments (member %d: need 0 < target < 1, 0 < lo <= hi, tolerance > "
                        "0, lo <= level <= hi, all finite)", e);
    }
    ON_DEVICE(h);
    if (upload_table(h, &h->policy, "rmt_n2_set_campaign_policy",
                     {{rows_host, (size_t)h->E * RMT_N2_POLICY_ROW * sizeof(double)}, {levels_host, (size_t)h->E * sizeof(double)}}))
        return 1;
    h->policy_comp = component;
    return 0;
}

extern "C" int rmt_n2_campaign_policy_step(rmt_n2_handle* h, void* y, double dt, double tol, int64_t max_iter,
                                           int max_evaluations, double* log_row, double* policy_row, rmt_n2_stats* stats) {
    if (!h || !y || !log_row || !policy_row || !stats) return fail("rmt_n2_campaign_policy_step: null argument");
    if (policy_ready(h, "rmt_n2_campaign_policy_step", true)) return 1;
    if (!(tol > 0) || max_iter < 1 || !(dt >= 0) || std::isinf(dt) || max_evaluations < 4)
        return fail("rmt_n2_campaign_policy_step: bad arguments (dt >= 0 and finite, tolerance > 0, max_iter >= 1, "
                    "max_evaluations >= 4)");
    if (h->fp32) return fail("rmt_n2_campaign_policy_step: fp64 only");
    ON_DEVICE(h);
    int N = h->N, E = h->E, comp = h->policy_comp;
    long long mi = (long long)max_iter;
    double* levels = policy_levels(h);
    void* args[] = {(void*)&y, (void*)&h->members.p, (void*)&N, (void*)&E, (void*)&tol, (void*)&mi, (void*)&stats,
                    (void*)&h->flags.p, (void*)&h->profile.p, (void*)&h->law.p, (void*)&dt, (void*)&log_row,
                    (void*)&h->policy.p, (void*)&levels, (void*)&policy_row, (void*)&comp, (void*)&max_evaluations};
    return launch_lanes(h, h->f_policy, args);
}

extern "C" int rmt_n2_get_campaign_level(rmt_n2_handle* h, double* levels_host) {
    if (!h || !levels_host) return fail("rmt_n2_get_campaign_level: null argument");
    if (policy_ready(h, "rmt_n2_get_campaign_level", true)) return 1;
    ON_DEVICE(h);
    HIP_OK(hipMemcpyAsync(levels_host, policy_levels(h), (size_t)h->E * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int rmt_n2_fallbacks(rmt_n2_handle* h, uint64_t* count) {
    if (!h || !count) return fail("null argument");
    ON_DEVICE(h);
    unsigned c = 0;
    HIP_OK(hipMemcpyAsync(&c, h->status_words() + h->E, sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    *count = c;
    return 0;
}

extern "C" int rmt_n2_status(rmt_n2_handle* h, uint32_t* flags_host) {
    if (!h || !flags_host) return fail("null argument");
    ON_DEVICE(h);
    HIP_OK(hipMemcpyAsync(flags_host, h->flags.p, (size_t)h->E * sizeof(unsigned), hipMemcpyDeviceToHost,
                          h->stream));
    HIP_OK(hipMemsetAsync(h->flags.p, 0, (size_t)h->E * sizeof(unsigned), h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------- side modules
// What the monitor, the controller and the fit share: a mechanism-independent module loaded on the device that was current
// at creation, one create and one destroy.
struct SideModule {
    int device = 0;
    hipModule_t module = nullptr;
    ~SideModule() {                          // (on the module's device: side_destroy switches to it, side_create has not left it)
        if (module) (void)hipModuleUnload(module);
    }
};
template <class M>
struct SideKernel { const char* name; hipFunction_t M::*f; };

// ``who``: the entry point, ``what``: "monitor" / "controller" / "fit", for the error texts; a module that lacks one of its
// kernels is unloaded again
template <class M>
static int side_create(const char* who, const char* what, const void* code, size_t size, M** out,
                       std::initializer_list<SideKernel<M>> kernels) {
    if (!code || !size || !out) return fail("%s: null argument", who);
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail("no HIP device available: the %s has no CPU fallback", what);
    std::unique_ptr<M> m(new M());
    hipError_t e = hipGetDevice(&m->device);
    if (e == hipSuccess) e = hipModuleLoadData(&m->module, code);
    for (const SideKernel<M>& k : kernels)
        if (e == hipSuccess) e = hipModuleGetFunction(&(m.get()->*k.f), m->module, k.name);
    if (e != hipSuccess) return fail("%s: %s", who, hipGetErrorString(e));
    *out = m.release();
    return 0;
}

template <class M>
static void side_destroy(M* m) {
    if (!m) return;
    DeviceGuard guard_(m->device);
    delete m;
}

// ---------------------------------------------------------------------------------------------- monitor
// Row reductions of a state in device memory (monitor_kernels.inc).  Independent of rmt_n2_handle: the code object is
// mechanism-independent, the sizes are run-time arguments.
// Layout of a reduce (measured on MI355X, profiles/monitor.md), 256 threads per workgroup:
//  * one WAVE per row (four rows per workgroup) for rows of at most RMT_N2_MONITOR_WAVE_BYTES, and for longer rows when
//    there are at least RMT_N2_MONITOR_ROWS_PER_CU rows per CU, one per SIMD: the waves alone fill the device
//    (2048 x 7 rows of 8 KiB: 19.7 us = 5.9 TB/s against 39 us with a workgroup per row);
//  * else one WORKGROUP per row (a few long rows; ONE 7 x 16384-node reactor: 6.3 us against 12.3 us by waves).
// The environment variables RMT_N2_MONITOR_WAVE_BYTES (rows up to this size by a wave, all others by a workgroup) and
// RMT_N2_MONITOR_BLOCK (threads of the workgroup-per-row form, up to 1024; 512 and 1024 measured slower as soon as there
// are more rows than CUs) replace the rule for measurements.
#define RMT_N2_MONITOR_BLOCK 256
#define RMT_N2_MONITOR_WGS_PER_CU 8       // grid cap: the rows beyond it are walked grid-stride
#define RMT_N2_MONITOR_WAVE_BYTES 8192
#define RMT_N2_MONITOR_ROWS_PER_CU 4

struct rmt_n2_monitor : SideModule {
    int n_cus = 0, last_rows_per_block = 0;
    hipFunction_t f64 = nullptr, f32 = nullptr;
};

extern "C" const char* rmt_n2_monitor_source(void) { return k_monitor_source; }
extern "C" void rmt_n2_monitor_destroy(rmt_n2_monitor* m) { side_destroy(m); }
extern "C" int rmt_n2_monitor_create(const void* code, size_t size, rmt_n2_monitor** out) {
    if (side_create("rmt_n2_monitor_create", "monitor", code, size, out,
                    {{"rmt_n2_monitor_rows_f64", &rmt_n2_monitor::f64}, {"rmt_n2_monitor_rows_f32", &rmt_n2_monitor::f32}}))
        return 1;
    const hipError_t e = hipDeviceGetAttribute(&(*out)->n_cus, hipDeviceAttributeMultiprocessorCount, (*out)->device);
    if (e == hipSuccess) return 0;
    side_destroy(*out);
    *out = nullptr;
    return fail("rmt_n2_monitor_create: %s", hipGetErrorString(e));
}

extern "C" int rmt_n2_monitor_reduce(rmt_n2_monitor* m, void* hip_stream, const void* y, const void* dydt_or_null,
                                     int E, int V, int N, int fp32, double* out) {
    if (!m || !y || !out) return fail("rmt_n2_monitor_reduce: null argument");
    if (E < 1 || V < 1 || N < 1) return fail("rmt_n2_monitor_reduce: bad sizes E=%d V=%d N=%d", E, V, N);
    const size_t real_size = fp32 ? 4 : 8;
    if (((size_t)y % real_size) || ((size_t)dydt_or_null % real_size) || ((size_t)out % sizeof(double)))
        return fail("rmt_n2_monitor_reduce: misaligned pointer");
    DeviceGuard guard_(m->device);
    if (guard_.err != hipSuccess)
        return fail("cannot switch to device %d of this monitor: %s", m->device, hipGetErrorString(guard_.err));
    static const long long env_wave_bytes = [] {  // tuning overrides, read once
        const char* v = getenv("RMT_N2_MONITOR_WAVE_BYTES");
        return v ? atoll(v) : -1LL;
    }();
    static const int env_block = [] {
        const char* v = getenv("RMT_N2_MONITOR_BLOCK");
        const int n = v ? atoi(v) : 0;
        return n >= 64 && n <= 1024 && n % 64 == 0 ? n : 0;
    }();
    long long rows = (long long)E * V;
    const long long row_bytes = (long long)N * (long long)real_size;
    const bool per_wave = env_wave_bytes >= 0 ? row_bytes <= env_wave_bytes
                                              : (row_bytes <= RMT_N2_MONITOR_WAVE_BYTES ||
                                                 rows >= (long long)m->n_cus * RMT_N2_MONITOR_ROWS_PER_CU);
    const int block = !per_wave && env_block ? env_block : RMT_N2_MONITOR_BLOCK;
    int rows_per_block = per_wave ? block / 64 : 1;
    long long grid = (rows + rows_per_block - 1) / rows_per_block;
    const long long cap = (long long)m->n_cus * RMT_N2_MONITOR_WGS_PER_CU;
    if (grid > cap) grid = cap;
    void* args[] = {(void*)&y, (void*)&dydt_or_null, (void*)&out, (void*)&rows, (void*)&N, (void*)&rows_per_block};
    if (launch((hipStream_t)hip_stream, fp32 ? m->f32 : m->f64, (size_t)grid, block, args)) return 1;
    m->last_rows_per_block = rows_per_block;
    return 0;
}

extern "C" int rmt_n2_monitor_last_rows_per_block(const rmt_n2_monitor* m) { return m ? m->last_rows_per_block : 0; }

// ---------------------------------------------------------------------------------------------- controller
// The sampled PI controller (control_kernels.inc): one kernel between two stepper launches, on the handle's stream.  One
// wave per member at 256 threads; at most RMT_N2_CONTROL_MAX_GRID workgroups (128 waves), the members beyond them are
// walked grid-stride - the kernel reads one row of the state per member at most and is latency-bound long before that.
#define RMT_N2_CONTROL_BLOCK 256
#define RMT_N2_CONTROL_MAX_GRID 32

struct rmt_n2_control : SideModule {
    hipFunction_t f_update = nullptr;
};

extern "C" const char* rmt_n2_control_source(void) { return k_control_source; }
extern "C" void rmt_n2_control_destroy(rmt_n2_control* c) { side_destroy(c); }
extern "C" int rmt_n2_control_create(const void* code, size_t size, rmt_n2_control** out) {
    return side_create("rmt_n2_control_create", "controller", code, size, out,
                       {{"rmt_n2_control_update_f64", &rmt_n2_control::f_update}});
}

extern "C" int rmt_n2_control_update(rmt_n2_control* c, rmt_n2_handle* h, const double* y, int V, int N,
                                     const double* params, const double* setpoint, double* state, double* log,
                                     int tail_at, int field, int hold) {
    if (!c || !h || !state) return fail("rmt_n2_control_update: null argument");
    if (!hold && (!y || !params || !setpoint || !log)) return fail("rmt_n2_control_update: null argument (update)");
    if (h->fp32) return fail("rmt_n2_control_update: fp64 handles only");
    if (h->device != c->device)
        return fail("rmt_n2_control_update: the handle lives on device %d, the controller on %d", h->device, c->device);
    const int width = RMT_N2_MEMBER_FIXED + h->S + h->NU;
    if (tail_at < RMT_N2_MEMBER_FIXED + h->S || tail_at + 4 > width)
        return fail("rmt_n2_control_update: the rows of this handle (%d doubles) carry no forcing tail at %d", width, tail_at);
    if (field < 0 || field > 2) return fail("rmt_n2_control_update: field must be 0, 1 or 2 (got %d)", field);
    if (!hold && (N < 1 || V < h->S || V > h->S + 1))
        return fail("rmt_n2_control_update: bad sizes V=%d N=%d for S=%d", V, N, h->S);
    if (((size_t)y | (size_t)params | (size_t)setpoint | (size_t)state | (size_t)log) % sizeof(double))
        return fail("rmt_n2_control_update: misaligned pointer");
    ON_DEVICE(h);
    int E = h->E, S = h->S;
    const int waves = RMT_N2_CONTROL_BLOCK / 64;
    int grid = (E + waves - 1) / waves;
    if (grid > RMT_N2_CONTROL_MAX_GRID) grid = RMT_N2_CONTROL_MAX_GRID;
    void* args[] = {(void*)&y,   (void*)&h->members.p, (void*)&params, (void*)&setpoint, (void*)&state,
                    (void*)&log, (void*)&E,            (void*)&S,      (void*)&V,        (void*)&N,
                    (void*)&width, (void*)&tail_at,    (void*)&field,  (void*)&hold};
    return launch(h->stream, c->f_update, grid, RMT_N2_CONTROL_BLOCK, args);
}

// ---------------------------------------------------------------------------------------------- fit
// Kinetic parameter estimation (fit_kernels.inc): the residual kernel - one wave per experiment at 256 threads, at most
// RMT_N2_FIT_MAX_GRID workgroups, the experiments beyond them walked grid-stride - and behind it the update kernel, ONE
// workgroup of one wave, on the handle's stream.
#define RMT_N2_FIT_BLOCK 256
#define RMT_N2_FIT_MAX_GRID 64
#define RMT_N2_FIT_MAX_PARAMS 8
#define RMT_N2_FIT_MAX_QUANTITIES 64

struct rmt_n2_fit : SideModule {
    hipFunction_t f_residuals = nullptr, f_update = nullptr, f_residuals_ex = nullptr, f_update_ex = nullptr;
};

extern "C" const char* rmt_n2_fit_source(void) { return k_fit_source; }
extern "C" void rmt_n2_fit_destroy(rmt_n2_fit* f) { side_destroy(f); }
extern "C" int rmt_n2_fit_create(const void* code, size_t size, rmt_n2_fit** out) {
    return side_create("rmt_n2_fit_create", "fit", code, size, out,
                       {{"rmt_n2_fit_residuals_f64", &rmt_n2_fit::f_residuals},
                        {"rmt_n2_fit_update_f64", &rmt_n2_fit::f_update},
                        {"rmt_n2_fit_residuals_ex_f64", &rmt_n2_fit::f_residuals_ex},
                        {"rmt_n2_fit_update_ex_f64", &rmt_n2_fit::f_update_ex}});
}

// rmt_n2_fit_step and rmt_n2_fit_step_ex: the same checks and the same two launches; ``who`` names the entry point in the
// error texts.  pos == nullptr: the plain pair of kernels.
static int fit_step(const char* who, rmt_n2_fit* f, rmt_n2_handle* h, const double* y, const double* sens,
                    const rmt_n2_stats* stats, int S, int V, int N, int n_params, const int* columns, const double* meas,
                    int MQ, double* contrib, double* pred, double* state, double* log_slice, double tolerance,
                    double damping0, const double* pos, const int* log_scale, const double* box) {
    const bool ex = pos != nullptr;
    if (!f || !h || !y || !sens || !stats || !columns || !meas || !contrib || !pred || !state || !log_slice)
        return fail("%s: null argument", who);
    if (n_params < 1 || n_params > RMT_N2_FIT_MAX_PARAMS) return fail("%s: 1..8 parameters (got %d)", who, n_params);
    if (!h->f_sens || !h->f_march)
        return fail("%s: this handle's code object is not the sensitivity unit (no rmt_n2_steady_sens beside "
                    "rmt_n2_steady_march)", who);
    if (h->fp32) return fail("%s: fp64 handles only", who);
    if (h->device != f->device)
        return fail("%s: the handle lives on device %d, the fit on %d", who, h->device, f->device);
    if (S != h->S || V != h->V || N != h->N)
        return fail("%s: S=%d V=%d N=%d are not the handle's (%d, %d, %d)", who, S, V, N, h->S, h->V, h->N);
    if (MQ < 1 || MQ > RMT_N2_FIT_MAX_QUANTITIES)
        return fail("%s: 1..%d measured quantities per experiment (got %d)", who, RMT_N2_FIT_MAX_QUANTITIES, MQ);
    if (!(tolerance >= 0) || !(damping0 > 0)) return fail("%s: tolerance >= 0 and damping > 0", who);
    struct { int col[RMT_N2_FIT_MAX_PARAMS]; } cols;
    struct { int col[RMT_N2_FIT_MAX_PARAMS]; int log[RMT_N2_FIT_MAX_PARAMS]; } scale;
    struct { double v[4][RMT_N2_FIT_MAX_PARAMS]; int log[RMT_N2_FIT_MAX_PARAMS]; } bx;
    std::memset(&cols, 0, sizeof(cols));
    std::memset(&scale, 0, sizeof(scale));
    std::memset(&bx, 0, sizeof(bx));
    for (int j = 0; j < n_params; ++j) {
        if (columns[j] < 0 || columns[j] >= h->NU)
            return fail("%s: parameter %d: user column %d is out of range (NU = %d)", who, j, columns[j], h->NU);
        cols.col[j] = scale.col[j] = columns[j];
    }
    if (ex) {
        if (N < 2) return fail("%s: positions along the bed need N >= 2 (got %d)", who, N);
        for (int j = 0; j < RMT_N2_FIT_MAX_PARAMS; ++j) {
            const bool in = j < n_params;
            scale.log[j] = bx.log[j] = in && log_scale[j] ? 1 : 0;
            for (int k = 0; k < 4; ++k)
                bx.v[k][j] = in ? box[k * RMT_N2_FIT_MAX_PARAMS + j] : (k % 2 ? HUGE_VAL : -HUGE_VAL);
            if (in && !(bx.v[0][j] < bx.v[1][j] && bx.v[2][j] < bx.v[3][j]))
                return fail("%s: parameter %d: the bounds must be lo < hi in p and in theta", who, j);
        }
    }
    if (((size_t)y | (size_t)sens | (size_t)stats | (size_t)meas | (size_t)contrib | (size_t)pred | (size_t)state |
         (size_t)log_slice | (size_t)pos) % sizeof(double))
        return fail("%s: misaligned pointer", who);
    ON_DEVICE(h);
    int E = h->E, width = RMT_N2_MEMBER_FIXED + h->S + h->NU;
    const int waves = RMT_N2_FIT_BLOCK / 64;
    int grid = (E + waves - 1) / waves;
    if (grid > RMT_N2_FIT_MAX_GRID) grid = RMT_N2_FIT_MAX_GRID;
    void* args1[] = {(void*)&y,    (void*)&sens,    (void*)&stats, (void*)&h->members.p, (void*)&meas,
                     (void*)&pred, (void*)&contrib, (void*)&E,     (void*)&S,            (void*)&V,
                     (void*)&N,    (void*)&n_params, (void*)&MQ,   (void*)&width,        (void*)&pos,
                     (void*)&scale};                  // (the plain kernel takes the first 14)
    if (launch(h->stream, ex ? f->f_residuals_ex : f->f_residuals, grid, RMT_N2_FIT_BLOCK, args1)) return 1;
    void* args2[] = {(void*)&contrib, (void*)&h->members.p, (void*)&state,    (void*)&log_slice, (void*)&E,
                     (void*)&S,       (void*)&n_params,     (void*)&width,    (void*)&cols,      (void*)&tolerance,
                     (void*)&damping0, (void*)&bx};   // (the plain kernel takes the first 11)
    return launch(h->stream, ex ? f->f_update_ex : f->f_update, 1, 64, args2);
}

extern "C" int rmt_n2_fit_step(rmt_n2_fit* f, rmt_n2_handle* h, const double* y, const double* sens,
                               const rmt_n2_stats* stats, int S, int V, int N, int n_params, const int* columns,
                               const double* meas, int MQ, double* contrib, double* pred, double* state, double* log_slice,
                               double tolerance, double damping0) {
    return fit_step("rmt_n2_fit_step", f, h, y, sens, stats, S, V, N, n_params, columns, meas, MQ, contrib, pred, state,
                    log_slice, tolerance, damping0, nullptr, nullptr, nullptr);
}

extern "C" int rmt_n2_fit_step_ex(rmt_n2_fit* f, rmt_n2_handle* h, const double* y, const double* sens,
                                  const rmt_n2_stats* stats, int S, int V, int N, int n_params, const int* columns,
                                  const double* meas, int MQ, double* contrib, double* pred, double* state,
                                  double* log_slice, double tolerance, double damping0, const double* pos,
                                  const int* log_scale, const double* box) {
    if (!pos || !log_scale || !box) return fail("rmt_n2_fit_step_ex: null argument");
    return fit_step("rmt_n2_fit_step_ex", f, h, y, sens, stats, S, V, N, n_params, columns, meas, MQ, contrib, pred, state,
                    log_slice, tolerance, damping0, pos, log_scale, box);
}
