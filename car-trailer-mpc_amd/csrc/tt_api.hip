// C-ABI boundary of libttmpc.so (declared in include/ttmpc.h).
//
// Host side of the drop-in: validates shapes before any launch (a mis-sized LDS or grid is a
// GPU fault), owns per-handle device workspaces for the host-pointer entry point, and forwards
// device-pointer calls straight to the kernel on the caller's stream.  No CPU fallback exists:
// every solve runs the gfx950 kernel in tt_track.hip.
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
#include <chrono>
#include <atomic>

#include "tt_kernel.hpp"
#include "ttmpc.h"

namespace {

// A device block that only grows.  A larger request waits for the device before the old block is freed (work that
// still reads it may be in flight on any stream); a failed allocation leaves the buffer empty.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    bool ensure(size_t bytes) {
        if (bytes <= cap) return true;
        if (p) {
            (void)hipDeviceSynchronize();
            (void)hipFree(p);
        }
        p = nullptr;
        cap = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            p = nullptr;
            return false;
        }
        cap = bytes;
        return true;
    }
};

struct Handle {
    tt_config cfg;
    double Q[36], R[4], xlb[6], xub[6], ulb[2], uub[2];
    double obs[4 * ttmpc::kObcaMaxM] = {};
    double dmin = 0.2;  // trajectory_optimization.py:95, mpc_control_obs.py:67 (tt_set_scene)
    int device = 0;
    hipStream_t stream = nullptr;
    // tracking host calls: one packed device input / output block and its pinned host mirror, so a
    // host-pointer solve is one H2D, the launch and one D2H (bytes).  The mirror is coherent (fine-grained) pinned
    // memory: small batches skip both copies and let the kernel read and write it in place (zd_*: its device view)
    size_t stage_in = 0, stage_out = 0;
    char *d_sin = nullptr, *d_sout = nullptr, *h_sin = nullptr, *h_sout = nullptr, *zd_sin = nullptr, *zd_sout = nullptr;
    std::string err;
    unsigned long long* obca_stamps = nullptr;  // diagnostics: per-phase clocks (ttx_obca_set_stamps)
    int nhelp = -1;                             // OBCA helper workgroups per launch (-1: one per CU; ttx_obca_set_helpers)
    unsigned long long spin_ticks = 0;          // hand-off spin limit (0: 5 s) and forced-timeout instance (-1: none),
    int fail_b = -1;                            //   ttx_obca_set_handoff_debug
    // Device workspaces, all under the one-stream rule of a handle's calls:
    DevBuf prow;   // tracking builds that keep stage rows in HBM (the N = 50 build, ttmpc::track_global_bytes)
    DevBuf dual;   // the multipliers of a tt_solve_batch_ex* call that asks for a sensitivity but not for them
    DevBuf xfer;   // the Stager's block: host arrays of tt_track_vjp, the _ex extras and the OBCA host calls
    DevBuf ows;    // OBCA solver workspace (HBM: ~1.8 MB per instance at N=200, M=6)
    DevBuf board;  // OBCA helper-workgroup board, one line per instance and a header line
};

thread_local std::string g_err;

// Makes the handle's device current for one entry point and restores the caller's device on every
// return path (the C ABI must not leave a different current device behind).
struct DeviceGuard {
    int prev = -1;
    hipError_t err;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev == device) {
            prev = -1;  // already current: nothing to switch or restore (a B = 1 call pays neither)
            err = hipSuccess;
        } else {
            err = hipSetDevice(device);
        }
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

int fail(Handle* h, int code, const char* fmt, const char* detail = "") {
    char buf[512];
    snprintf(buf, sizeof buf, fmt, detail);
    if (h) h->err = buf;
    g_err = buf;
    return code;
}

int hip_fail(Handle* h, hipError_t e, const char* where) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s: %s", where, hipGetErrorString(e));
    if (h) h->err = buf;
    g_err = buf;
    return -EIO;
}

int no_memory(Handle* h, const char* what) { return fail(h, -ENOMEM, "%s allocation failed", what); }

bool is_obca(const tt_config& c) { return c.variant == TT_VARIANT_TRACK_OBCA || c.variant == TT_VARIANT_OBCA_PLAN; }

// ---------------- the prelude of every entry point ----------------
// The checks an entry asks for run in this order: handle, variant class, sign of B, empty batch, fuzzy weights, size of
// B.  An entry whose own checks (its pointers) sit between two of them asks in two steps.  Returns 0 to go on, an
// error code, or kEmptyBatch (the entry returns 0 without touching anything): `if (rc) return result(rc);`.
enum : unsigned {
    kHandle = 1, kTrackOnly = 2, kObcaOnly = 4, kPlanOnly = 8, kNotPlan = 16, kSign = 32, kEmpty = 64, kFuzzy = 128,
    kRange = 256
};
constexpr int kEmptyBatch = 1;
int result(int rc) { return rc == kEmptyBatch ? 0 : rc; }

int prelude(Handle* h, int B, unsigned checks, const void* weights = nullptr, int max_b = 1 << 30) {
    if (!h) return fail(nullptr, -EINVAL, "NULL handle%s");
    if ((checks & kTrackOnly) && is_obca(h->cfg))
        return fail(h, -EINVAL, "multipliers and sensitivities are exported by the tracking variants only%s");
    if ((checks & kObcaOnly) && !is_obca(h->cfg)) return fail(h, -EINVAL, "handle is not an OBCA variant%s");
    if ((checks & kPlanOnly) && h->cfg.variant != TT_VARIANT_OBCA_PLAN)
        return fail(h, -EINVAL, "tt_plan_batch needs a TT_VARIANT_OBCA_PLAN handle%s");
    if ((checks & kNotPlan) && h->cfg.variant == TT_VARIANT_OBCA_PLAN)
        return fail(h, -EINVAL, "plan handles solve through tt_plan_batch / tt_obca_solve_batch%s");
    if ((checks & kSign) && B < 0) return fail(h, -EINVAL, "B must be >= 0%s");
    if ((checks & kEmpty) && B == 0) return kEmptyBatch;
    if ((checks & kFuzzy) && h->cfg.variant == TT_VARIANT_FUZZY && !weights)
        return fail(h, -EINVAL, "fuzzy variant needs per-instance weights (mpc_control_fuzzy.py:54-58)%s");
    if ((checks & kRange) && B > max_b) return fail(h, -EINVAL, "B too large%s");
    return 0;
}

// ---------------- host staging ----------------
// Host arrays of one call behind one device block: register the arrays (absent ones get a NULL device pointer and no
// memory), carve the block, enqueue the uploads, launch, enqueue the downloads.  err keeps the first failed copy.
class Stager {
  public:
    hipError_t err = hipSuccess;
    // an input: copied to the device if the host has it
    template <class T>
    void in(const T* host, size_t count, const T** dev) {
        add(host, nullptr, count * sizeof(T), host != nullptr, (void**)dev);
    }
    // an output: copied back if the host wants it; device_only: the launch needs the array even if the host does not
    template <class T>
    void out(T* host, size_t count, T** dev, bool device_only = false) {
        add(nullptr, host, count * sizeof(T), host != nullptr || device_only, (void**)dev);
    }
    // an accumulator: copied to the device and back if the host has it
    template <class T>
    void inout(T* host, size_t count, T** dev) {
        add(host, host, count * sizeof(T), host != nullptr, (void**)dev);
    }
    bool carve(DevBuf& buf) {
        if (!buf.ensure(total_)) return false;
        for (int t = 0; t < n_; ++t)
            if (it_[t].used) *it_[t].dev = static_cast<char*>(buf.p) + it_[t].off;
        return true;
    }
    void upload(hipStream_t s) { copy(s, true); }
    void download(hipStream_t s) { copy(s, false); }
    // The tail of a host call, after carve(): the uploads, device() (the call's device entry on s; it has set the error
    // text if it fails), the downloads and the stream wait.  The first error wins; `what` names a failed copy or wait.
    template <class Device>
    int run(Handle* h, hipStream_t s, const char* what, Device device) {
        upload(s);
        if (err != hipSuccess) {
            (void)hipStreamSynchronize(s);
            return hip_fail(h, err, "H2D copy");
        }
        if (const int rc = device()) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        download(s);
        const hipError_t es = hipStreamSynchronize(s);
        const hipError_t e = err != hipSuccess ? err : es;
        return e != hipSuccess ? hip_fail(h, e, what) : 0;
    }

  private:
    struct Item {
        const void* h2d;
        void* d2h;
        size_t bytes, off;
        bool used;
        void** dev;
    };
    static constexpr int kMax = 20;  // (tt_obca_vjp_geometry registers 17)
    Item it_[kMax];
    int n_ = 0;
    size_t total_ = 0;

    void add(const void* h2d, void* d2h, size_t bytes, bool used, void** dev) {
        if (n_ == kMax) abort();  // (a fixed list per entry point: never at run time)
        *dev = nullptr;
        it_[n_++] = Item{h2d, d2h, bytes, total_, used, dev};
        if (used) total_ += (bytes + 255) & ~(size_t)255;  // every array as aligned as an allocation of its own
    }
    void copy(hipStream_t s, bool up) {
        for (int t = 0; t < n_; ++t) {
            const Item& i = it_[t];
            if (err != hipSuccess || !i.used || !(up ? i.h2d != nullptr : i.d2h != nullptr)) continue;
            err = up ? hipMemcpyAsync(*i.dev, i.h2d, i.bytes, hipMemcpyHostToDevice, s)
                     : hipMemcpyAsync(i.d2h, *i.dev, i.bytes, hipMemcpyDeviceToHost, s);
        }
    }
};

// tt_track_vjp_out as the model entries take it, in o: no g_model.  NULL stays NULL (theirs to refuse).
const tt_track_vjp_model_out* widen(const tt_track_vjp_out* out, tt_track_vjp_model_out& o) {
    if (!out) return nullptr;
    o = {out->g_x0, out->g_xref, out->g_uref, out->g_wq_wr, nullptr, out->vjp_status};
    return &o;
}

// tt_track_vjp_model_out as the bounds entries take it, in o: no g_bounds.  NULL stays NULL (theirs to refuse).
const tt_track_vjp_bounds_out* widen(const tt_track_vjp_model_out* out, tt_track_vjp_bounds_out& o) {
    if (!out) return nullptr;
    o = {out->g_x0, out->g_xref, out->g_uref, out->g_wq_wr, out->g_model, nullptr, out->vjp_status};
    return &o;
}

// ---------------- the zero-copy mirror of tracking host calls ----------------
void free_stage(Handle* h) {
    if (h->d_sin) (void)hipFree(h->d_sin);
    if (h->d_sout) (void)hipFree(h->d_sout);
    if (h->h_sin) (void)hipHostFree(h->h_sin);
    if (h->h_sout) (void)hipHostFree(h->h_sout);
    h->d_sin = h->d_sout = h->h_sin = h->h_sout = h->zd_sin = h->zd_sout = nullptr;
    h->stage_in = h->stage_out = 0;
}

int ensure_stage(Handle* h, size_t in_bytes, size_t out_bytes) {
    if (in_bytes <= h->stage_in && out_bytes <= h->stage_out) return 0;
    // a zero-copy call returns once its statuses are written, before its kernel has retired: let it retire first
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_stage(h);
    hipError_t e = hipMalloc((void**)&h->d_sin, in_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&h->d_sout, out_bytes);
    // coherent: the GPU does not cache these pages, so a kernel reading the mirror in place sees this call's inputs
    // (not an L2 copy of the previous call's) and its output stores are in host memory when the stream completes
    const unsigned fl = hipHostMallocMapped | hipHostMallocCoherent | hipHostMallocPortable;
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_sin, in_bytes, fl);
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_sout, out_bytes, fl);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&h->zd_sin, h->h_sin, 0);
    if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&h->zd_sout, h->h_sout, 0);
    if (e != hipSuccess) {
        free_stage(h);
        return fail(h, -ENOMEM, "staging allocation failed (%s bytes)", std::to_string(in_bytes + out_bytes).c_str());
    }
    h->stage_in = in_bytes;
    h->stage_out = out_bytes;
    return 0;
}

// Largest batch a host-pointer tracking solve runs zero-copy (the kernel reads its inputs from and writes its outputs
// to the coherent pinned mirror; no H2D / D2H on the stream).  Only where the kernel reads its inputs once, at load
// (N < 64: the reference window lives in registers, tt_track.hip regref).  TT_ZERO_COPY_MAX overrides (0: off).
int zero_copy_max() {
    static const int v = [] {
        const char* e = getenv("TT_ZERO_COPY_MAX");
        return e ? atoi(e) : 64;
    }();
    return v;
}

// a status value no kernel writes: the zero-copy path's "not finished yet"
constexpr int kStatusPending = -0x40000000;

// Wait until every instance of a zero-copy call has written its status (host memory; the kernel's release orders the
// instance's other outputs before it).  Spins up to 2 ms, then yields to the OS between looks; gives up after 1 s, and
// the caller then waits for the stream (which also reports a fault that kept a status from ever being written).
bool poll_done(volatile int* st, int B) {
    const auto t0 = std::chrono::steady_clock::now();
    for (long long n = 0;; ++n) {
        int i = 0;
        while (i < B && st[i] != kStatusPending) ++i;
        if (i == B) {
            std::atomic_thread_fence(std::memory_order_acquire);
            return true;
        }
        if ((n & 255) == 255) {
            const auto dt = std::chrono::steady_clock::now() - t0;
            if (dt > std::chrono::seconds(1)) return false;
            if (dt > std::chrono::milliseconds(2)) std::this_thread::yield();
        }
    }
}

void defaults(tt_config& c) {
    const bool relaxed = c.variant == TT_VARIANT_NMPC || c.variant == TT_VARIANT_FUZZY;
    // IPOPT options of the reference classes: mpc_control.py:35-39 (defaults tol 1e-8, acceptable
    // 1e-6 x 15), mpc_control_nmpc.py:36-45 / mpc_control_fuzzy.py:47-58 (tol 1e-3, acc 1e-2 x 5),
    // mpc_control_obs.py:189-193 / trajectory_optimization.py:196-199 (max_iter 5000, IPOPT defaults)
    if (c.tol <= 0) c.tol = relaxed ? 1e-3 : 1e-8;
    if (c.acc_tol <= 0) c.acc_tol = relaxed ? 1e-2 : 1e-6;
    if (c.max_iter <= 0) c.max_iter = relaxed ? 2000 : 5000;
    if (c.acc_iter <= 0) c.acc_iter = relaxed ? 5 : 15;
}

// ---------------- kernel arguments ----------------
// the model block every args struct carries under the same names
template <class Args>
void fill_model(Args& a, const Handle* h) {
    a.dt = h->cfg.dt;
    a.L1 = h->cfg.L1;
    a.L2 = h->cfg.L2;
    a.Mh = h->cfg.Mh;
    memcpy(a.Q, h->Q, sizeof a.Q);
    memcpy(a.R, h->R, sizeof a.R);
    memcpy(a.xlb, h->xlb, sizeof a.xlb);
    memcpy(a.xub, h->xub, sizeof a.xub);
    memcpy(a.ulb, h->ulb, sizeof a.ulb);
    memcpy(a.uub, h->uub, sizeof a.uub);
}

// a tracking launch without its arrays; the launch's HBM stage rows come from the handle
int make_track_args(Handle* h, int B, ttmpc::TrackArgs& a) {
    memset(&a, 0, sizeof a);
    a.N = h->cfg.N;
    a.B = B;
    a.max_iter = h->cfg.max_iter;
    a.acc_iter = h->cfg.acc_iter;
    a.tol = h->cfg.tol;
    a.acc_tol = h->cfg.acc_tol;
    fill_model(a, h);
    if (const size_t gb = ttmpc::track_global_bytes(a)) {
        if (!h->prow.ensure(gb)) return no_memory(h, "stage-row workspace");
        a.prow = static_cast<double*>(h->prow.p);
    }
    return 0;
}

// SensArgs / VjpArgs with their common head filled
template <class Args>
Args diff_args(const Handle* h, int B, const double* d_x, const double* d_u, const double* d_dual,
               const double* d_wq_wr, const int* d_status) {
    Args a{};
    a.N = h->cfg.N;
    a.B = B;
    fill_model(a, h);
    a.x = d_x;
    a.u = d_u;
    a.dual = d_dual;
    a.wqwr = d_wq_wr;
    a.status = d_status;
    return a;
}

// ---------------- tracking solves ----------------
int solve_device_impl(Handle* h, int B, const double* d_x0, const double* d_xref, const double* d_uref,
                      const double* d_wq_wr, const double* d_z_guess, double* d_x_out, double* d_u_out, int* d_status,
                      int* d_iters, double* d_kkt_res, void* stream, int host_done, double* d_dual = nullptr) {
    if (const int rc = prelude(h, B, kHandle | kSign | kEmpty | kRange)) return result(rc);
    if (!d_x0 || !d_xref || !d_uref || !d_x_out || !d_u_out || !d_status)
        return fail(h, -EINVAL, "NULL device buffer%s");
    if (const int rc = prelude(h, B, kNotPlan)) return rc;
    if (h->cfg.variant == TT_VARIANT_TRACK_OBCA)
        return tt_obca_solve_batch_device(h, B, d_x0, nullptr, d_xref, d_uref, d_z_guess, d_x_out, d_u_out, nullptr,
                                          d_status, d_iters, d_kkt_res, stream);
    if (const int rc = prelude(h, B, kFuzzy, d_wq_wr)) return rc;
    DeviceGuard dg(h->device);
    if (dg.err != hipSuccess) return hip_fail(h, dg.err, "hipSetDevice");
    ttmpc::TrackArgs a;
    if (const int rc = make_track_args(h, B, a)) return rc;
    a.x0 = d_x0;
    a.xref = d_xref;
    a.uref = d_uref;
    a.wqwr = d_wq_wr;
    a.zg = d_z_guess;
    a.xout = d_x_out;
    a.uout = d_u_out;
    a.kkt = d_kkt_res;
    a.status = d_status;
    a.iters = d_iters;
    a.host_done = host_done;
    a.dual = d_dual;
    const hipError_t e = ttmpc::launch_track(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(h, e, "track kernel launch");
    return 0;
}

bool wants_sens(const tt_track_extra& x) { return x.gain || x.dxdx0 || x.dudx0 || x.sens_status; }
bool wants_any(const tt_track_extra* x) { return x && (x->dual || wants_sens(*x)); }

// the sensitivity launch behind both entry points; the caller has made the handle's device current
int sens_launch(Handle* h, int B, const double* d_x, const double* d_u, const double* d_dual, const double* d_wq_wr,
                const int* d_status, const tt_track_extra& x, void* stream) {
    ttmpc::SensArgs a = diff_args<ttmpc::SensArgs>(h, B, d_x, d_u, d_dual, d_wq_wr, d_status);
    a.gain = x.gain;
    a.dxdx0 = x.dxdx0;
    a.dudx0 = x.dudx0;
    a.sens_status = x.sens_status;
    const hipError_t e = ttmpc::launch_track_sens(a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(h, e, "sensitivity kernel launch");
    return 0;
}

// solve (+ multiplier export) and, if asked for, the sensitivity launch behind it on the same stream
int ex_device_impl(Handle* h, int B, const double* d_x0, const double* d_xref, const double* d_uref,
                   const double* d_wq_wr, const double* d_z_guess, double* d_x_out, double* d_u_out, int* d_status,
                   int* d_iters, double* d_kkt_res, const tt_track_extra& x, void* stream) {
    if (const int rc = prelude(h, B, kHandle | kTrackOnly | kSign | kEmpty)) return result(rc);
    const bool sens = wants_sens(x);
    double* d_dual = x.dual;
    DeviceGuard dg(h->device);
    if (dg.err != hipSuccess) return hip_fail(h, dg.err, "hipSetDevice");
    if (sens && !d_dual) {
        if (!h->dual.ensure((size_t)B * (h->cfg.N + 1) * ttmpc::kDualPerStage * sizeof(double)))
            return no_memory(h, "multiplier workspace");
        d_dual = static_cast<double*>(h->dual.p);
    }
    const int rc = solve_device_impl(h, B, d_x0, d_xref, d_uref, d_wq_wr, d_z_guess, d_x_out, d_u_out, d_status,
                                     d_iters, d_kkt_res, stream, 0, d_dual);
    if (rc || !sens) return rc;
    return sens_launch(h, B, d_x_out, d_u_out, d_dual, d_wq_wr, d_status, x, stream);
}

int solve_host(Handle* h, int B, const double* x0, const double* xref, const double* uref, const double* wq_wr,
               const double* z_guess, double* x_out, double* u_out, int* status, int* iters, double* kkt_res,
               const tt_track_extra* extra) {
    if (const int rc = prelude(h, B, kHandle | kSign | kEmpty)) return result(rc);
    if (!x0 || !xref || !uref || !x_out || !u_out || !status) return fail(h, -EINVAL, "NULL host buffer%s");
    if (const int rc = prelude(h, B, kNotPlan)) return rc;
    if (is_obca(h->cfg)) {  // MPC+OBCA handle: its own host path (workspace, z_guess layout)
        if (extra) return prelude(h, B, kTrackOnly);
        return tt_obca_solve_batch(h, B, x0, nullptr, xref, uref, z_guess, x_out, u_out, nullptr, status, iters,
                                   kkt_res);
    }
    // validate everything tt_solve_batch_device would refuse before the staging buffer is touched
    if (const int rc = prelude(h, B, kFuzzy | kRange, wq_wr)) return rc;
    DeviceGuard dg(h->device);
    hipError_t e = dg.err;
    if (e != hipSuccess) return hip_fail(h, e, "hipSetDevice");
    // packed layout, instance-major within each array: in  = x0 | xref | uref | [wq_wr] | [z_guess]
    //                                                   out = X | U | kkt | status, iters (int32)
    const size_t N = h->cfg.N, b = (size_t)B, nz = 8 * N + 6;
    const size_t sizes[5] = {b * 6, b * (N + 1) * 6, b * N * 2, wq_wr ? b * 8 : 0, z_guess ? b * nz : 0};
    const double* srcs[5] = {x0, xref, uref, wq_wr, z_guess};
    size_t in_d = 0;
    for (size_t v : sizes) in_d += v;
    const size_t nxo = b * (N + 1) * 6, nuo = b * N * 2, out_d = nxo + nuo + b + b;  // 2 x int32 per instance = 1 double
    int rc = ensure_stage(h, in_d * 8, out_d * 8);
    if (rc) return rc;
    // the extra outputs of tt_solve_batch_ex, straight into the caller's arrays (a call that asks for a sensitivity
    // always has the multipliers on the device)
    Stager ex;
    tt_track_extra dx = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (extra) {
        ex.out(extra->dual, b * (N + 1) * ttmpc::kDualPerStage, &dx.dual, true);
        ex.out(extra->gain, b * 12, &dx.gain);
        ex.out(extra->dxdx0, b * (N + 1) * 36, &dx.dxdx0);
        ex.out(extra->dudx0, b * N * 12, &dx.dudx0);
        ex.out(extra->sens_status, b, &dx.sens_status);
        if (!ex.carve(h->xfer)) return no_memory(h, "extra-output workspace");
    }
    // zero-copy for small batches (B = 1 latency: the two DMA copies cost more than the kernel's few PCIe reads); a call
    // with extra outputs always copies (they are not part of the coherent mirror)
    const bool zc = !extra && B <= zero_copy_max() && N < 64;
    double* hin = reinterpret_cast<double*>(h->h_sin);
    const double* dptr[5];
    size_t off = 0;
    for (int a = 0; a < 5; ++a) {
        if (sizes[a]) memcpy(hin + off, srcs[a], sizes[a] * 8);
        dptr[a] = reinterpret_cast<const double*>(zc ? h->zd_sin : h->d_sin) + off;
        off += sizes[a];
    }
    hipStream_t s = h->stream;
    if (!zc) {
        e = hipMemcpyAsync(h->d_sin, h->h_sin, in_d * 8, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return hip_fail(h, e, "H2D copy");
    }
    double* dxo = reinterpret_cast<double*>(zc ? h->zd_sout : h->d_sout);
    double* duo = dxo + nxo;
    double* dkk = duo + nuo;
    int* dst = reinterpret_cast<int*>(dkk + b);
    int* dit = dst + b;
    // zero-copy: status[] in the host block doubles as the instances' completion flags (the kernel writes each last,
    // behind a system-scope release); a pending sentinel, then a poll of host memory instead of the stream wait
    volatile int* hst = zc ? reinterpret_cast<volatile int*>(h->h_sout + (nxo + nuo + b) * 8) : nullptr;
    if (zc)
        for (int i = 0; i < B; ++i) hst[i] = kStatusPending;
    if (extra)
        rc = ex_device_impl(h, B, dptr[0], dptr[1], dptr[2], wq_wr ? dptr[3] : nullptr, z_guess ? dptr[4] : nullptr, dxo,
                            duo, dst, dit, dkk, dx, s);
    else
        rc = solve_device_impl(h, B, dptr[0], dptr[1], dptr[2], wq_wr ? dptr[3] : nullptr, z_guess ? dptr[4] : nullptr,
                               dxo, duo, dst, dit, dkk, s, zc ? 1 : 0);
    if (rc) {
        (void)hipStreamSynchronize(s);  // the H2D from the pinned staging buffer may still be in flight
        return rc;
    }
    bool done = false;
    if (zc) done = poll_done(hst, B);
    e = zc ? hipSuccess : hipMemcpyAsync(h->h_sout, h->d_sout, out_d * 8, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) {  // (the stream wait below covers the extras too)
        ex.download(s);
        e = ex.err;
    }
    if (e == hipSuccess && !done) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        return hip_fail(h, e, "solve");
    }
    const double* ho = reinterpret_cast<const double*>(h->h_sout);
    memcpy(x_out, ho, nxo * 8);
    memcpy(u_out, ho + nxo, nuo * 8);
    if (kkt_res) memcpy(kkt_res, ho + nxo + nuo, b * 8);
    const int* hi = reinterpret_cast<const int*>(ho + nxo + nuo + b);
    memcpy(status, hi, b * 4);
    if (iters) memcpy(iters, hi + b, b * 4);
    return 0;
}

}  // namespace

extern "C" {

int tt_create(const tt_config* cfg, const double* Q, const double* R, const double* xlb, const double* xub,
              const double* ulb, const double* uub, const double* obstacles, int device, void** handle) {
    if (!handle) return fail(nullptr, -EINVAL, "handle pointer is NULL%s");
    *handle = nullptr;
    if (!cfg || !Q || !R || !xlb || !xub || !ulb || !uub) return fail(nullptr, -EINVAL, "NULL argument%s");
    if (cfg->nx != 6 || cfg->nu != 2)
        return fail(nullptr, -EINVAL, "truck-trailer model has nx=6, nu=2 (truck_trailer_model.py:4-5)%s");
    const bool obca = is_obca(*cfg);
    if (!obca && cfg->variant != TT_VARIANT_TRACK && cfg->variant != TT_VARIANT_NMPC && cfg->variant != TT_VARIANT_FUZZY)
        return fail(nullptr, -EINVAL, "unknown variant%s");
    if (obca) {
        // mpc_control_obs.py:149 / trajectory_optimization.py:25-26 need at least one obstacle
        if (cfg->M < 1 || cfg->M > ttmpc::kObcaMaxM)
            return fail(nullptr, -EINVAL, "OBCA variants need 1 <= M <= %s obstacles",
                        std::to_string(ttmpc::kObcaMaxM).c_str());
        if (!obstacles) return fail(nullptr, -EINVAL, "OBCA variants need the obstacle list (M x [cx, cy, w, h])%s");
        if (cfg->N < 1 || cfg->N > 100000) return fail(nullptr, -EINVAL, "horizon must be in [1, 100000]%s");
        if (!(cfg->W1 > 0) || !(cfg->W2 > 0)) return fail(nullptr, -EINVAL, "params W1, W2 must be > 0%s");
        for (int i = 0; i < 4 * cfg->M; ++i)
            if (!isfinite(obstacles[i])) return fail(nullptr, -EINVAL, "non-finite obstacle entry%s");
    } else if (cfg->N < 1 || cfg->N > ttmpc::max_horizon()) {
        return fail(nullptr, -EINVAL, "horizon must be in [1, %s] (LDS-resident instance)",
                    std::to_string(ttmpc::max_horizon()).c_str());
    }
    if (!(cfg->dt > 0) || !(cfg->L1 > 0) || !(cfg->L2 > 0) || !isfinite(cfg->Mh))
        return fail(nullptr, -EINVAL, "params dt, L1, L2 must be > 0 and M finite%s");
    for (int i = 0; i < 6; ++i)
        if (!(xlb[i] <= xub[i])) return fail(nullptr, -EINVAL, "state bound lb > ub%s");
    for (int i = 0; i < 2; ++i)
        if (!(ulb[i] <= uub[i])) return fail(nullptr, -EINVAL, "input bound lb > ub%s");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, -ENODEV, "no HIP device: ttmpc is GPU-only (gfx950)%s");
    if (device < 0 || device >= ndev) return fail(nullptr, -ENODEV, "device ordinal out of range%s");
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, -ENODEV, "device is not gfx950 (MI355X): %s", prop.gcnArchName);
    Handle* h = new Handle();
    h->cfg = *cfg;
    defaults(h->cfg);
    memcpy(h->Q, Q, sizeof h->Q);
    memcpy(h->R, R, sizeof h->R);
    memcpy(h->xlb, xlb, sizeof h->xlb);
    memcpy(h->xub, xub, sizeof h->xub);
    memcpy(h->ulb, ulb, sizeof h->ulb);
    memcpy(h->uub, uub, sizeof h->uub);
    if (obca) memcpy(h->obs, obstacles, sizeof(double) * 4 * cfg->M);
    h->device = device;
    DeviceGuard dg(device);
    hipError_t e = dg.err;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        int rc = hip_fail(nullptr, e, "tt_create");
        delete h;
        return rc;
    }
    *handle = h;
    return 0;
}

int tt_solve_batch_device(void* handle, int B, const double* d_x0, const double* d_xref, const double* d_uref,
                          const double* d_wq_wr, const double* d_z_guess, double* d_x_out, double* d_u_out,
                          int* d_status, int* d_iters, double* d_kkt_res, void* stream) {
    return solve_device_impl(static_cast<Handle*>(handle), B, d_x0, d_xref, d_uref, d_wq_wr, d_z_guess, d_x_out,
                             d_u_out, d_status, d_iters, d_kkt_res, stream, 0);
}

int tt_solve_batch(void* handle, int B, const double* x0, const double* xref, const double* uref,
                   const double* wq_wr, const double* z_guess, double* x_out, double* u_out, int* status,
                   int* iters, double* kkt_res) {
    return solve_host(static_cast<Handle*>(handle), B, x0, xref, uref, wq_wr, z_guess, x_out, u_out, status, iters,
                      kkt_res, nullptr);
}

int tt_solve_batch_ex(void* handle, int B, const double* x0, const double* xref, const double* uref,
                      const double* wq_wr, const double* z_guess, double* x_out, double* u_out, int* status,
                      int* iters, double* kkt_res, const tt_track_extra* extra) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, B, kHandle | kTrackOnly)) return rc;
    return solve_host(h, B, x0, xref, uref, wq_wr, z_guess, x_out, u_out, status, iters, kkt_res,
                      wants_any(extra) ? extra : nullptr);
}

int tt_solve_batch_ex_device(void* handle, int B, const double* d_x0, const double* d_xref, const double* d_uref,
                             const double* d_wq_wr, const double* d_z_guess, double* d_x_out, double* d_u_out,
                             int* d_status, int* d_iters, double* d_kkt_res, const tt_track_extra* d_extra,
                             void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, B, kHandle | kTrackOnly)) return rc;
    if (!wants_any(d_extra))
        return solve_device_impl(h, B, d_x0, d_xref, d_uref, d_wq_wr, d_z_guess, d_x_out, d_u_out, d_status, d_iters,
                                 d_kkt_res, stream, 0);
    return ex_device_impl(h, B, d_x0, d_xref, d_uref, d_wq_wr, d_z_guess, d_x_out, d_u_out, d_status, d_iters,
                          d_kkt_res, *d_extra, stream);
}

int tt_track_sens_device(void* handle, int B, const double* d_x, const double* d_u, const double* d_dual,
                         const double* d_wq_wr, const int* d_status, double* d_gain, double* d_dxdx0,
                         double* d_dudx0, int* d_sens_status, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, B, kHandle | kTrackOnly | kSign | kEmpty | kRange)) return result(rc);
    if (!d_x || !d_u || !d_dual || !d_status) return fail(h, -EINVAL, "NULL device buffer%s");
    if (const int rc = prelude(h, B, kFuzzy, d_wq_wr)) return rc;
    DeviceGuard dg(h->device);
    if (dg.err != hipSuccess) return hip_fail(h, dg.err, "hipSetDevice");
    const tt_track_extra x = {nullptr, d_gain, d_dxdx0, d_dudx0, d_sens_status};
    return sens_launch(h, B, d_x, d_u, d_dual, d_wq_wr, d_status, x, stream);
}

int tt_track_vjp_bounds_device(void* handle, int B, const double* d_x, const double* d_u, const double* d_dual,
                               const double* d_xref, const double* d_uref, const double* d_wq_wr, const int* d_status,
                               const double* d_grad_x, const double* d_grad_u, const tt_track_vjp_bounds_out* d_out,
                               int accumulate, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, B, kHandle | kTrackOnly | kSign)) return rc;
    if (!d_grad_x && !d_grad_u) return fail(h, -EINVAL, "grad_x and grad_u are both NULL: no loss to differentiate%s");
    if (const int rc = prelude(h, B, kEmpty | kRange)) return result(rc);
    if (!d_x || !d_u || !d_dual || !d_status || !d_out) return fail(h, -EINVAL, "NULL device buffer%s");
    if (d_out->g_wq_wr && (!d_xref || !d_uref))
        return fail(h, -EINVAL, "the weight gradient needs xref and uref of the solve%s");
    if (const int rc = prelude(h, B, kFuzzy, d_wq_wr)) return rc;
    DeviceGuard dg(h->device);
    if (dg.err != hipSuccess) return hip_fail(h, dg.err, "hipSetDevice");
    ttmpc::VjpBoundsArgs a = diff_args<ttmpc::VjpBoundsArgs>(h, B, d_x, d_u, d_dual, d_wq_wr, d_status);
    a.xref = d_xref;
    a.uref = d_uref;
    a.gx = d_grad_x;
    a.gu = d_grad_u;
    a.g_x0 = d_out->g_x0;
    a.g_xref = d_out->g_xref;
    a.g_uref = d_out->g_uref;
    a.g_wqwr = d_out->g_wq_wr;
    a.vjp_status = d_out->vjp_status;
    a.g_model = d_out->g_model;
    a.accumulate = accumulate != 0;
    a.g_bounds = d_out->g_bounds;
    // without g_bounds the model instantiation, without g_model either the plain one: on the VjpModelArgs / VjpArgs
    // head of the same block
    hipStream_t s = static_cast<hipStream_t>(stream);
    const hipError_t e = a.g_bounds ? ttmpc::launch_track_vjp_bounds(a, s)
                         : a.g_model ? ttmpc::launch_track_vjp_model(a, s) : ttmpc::launch_track_vjp(a, s);
    if (e != hipSuccess) return hip_fail(h, e, "adjoint kernel launch");
    return 0;
}

int tt_track_vjp_model_device(void* handle, int B, const double* d_x, const double* d_u, const double* d_dual,
                              const double* d_xref, const double* d_uref, const double* d_wq_wr, const int* d_status,
                              const double* d_grad_x, const double* d_grad_u, const tt_track_vjp_model_out* d_out,
                              int accumulate, void* stream) {
    tt_track_vjp_bounds_out o;
    return tt_track_vjp_bounds_device(handle, B, d_x, d_u, d_dual, d_xref, d_uref, d_wq_wr, d_status, d_grad_x,
                                      d_grad_u, widen(d_out, o), accumulate, stream);
}

int tt_track_vjp_device(void* handle, int B, const double* d_x, const double* d_u, const double* d_dual,
                        const double* d_xref, const double* d_uref, const double* d_wq_wr, const int* d_status,
                        const double* d_grad_x, const double* d_grad_u, const tt_track_vjp_out* d_out, void* stream) {
    tt_track_vjp_model_out o;
    return tt_track_vjp_model_device(handle, B, d_x, d_u, d_dual, d_xref, d_uref, d_wq_wr, d_status, d_grad_x,
                                     d_grad_u, widen(d_out, o), 0, stream);
}

int tt_track_vjp_bounds(void* handle, int B, const double* x, const double* u, const double* dual, const double* xref,
                        const double* uref, const double* wq_wr, const int* status, const double* grad_x,
                        const double* grad_u, const tt_track_vjp_bounds_out* out, int accumulate) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, B, kHandle | kTrackOnly | kSign)) return rc;
    if (!grad_x && !grad_u) return fail(h, -EINVAL, "grad_x and grad_u are both NULL: no loss to differentiate%s");
    if (const int rc = prelude(h, B, kEmpty | kRange)) return result(rc);
    if (!x || !u || !dual || !status || !out) return fail(h, -EINVAL, "NULL host buffer%s");
    DeviceGuard dg(h->device);
    if (dg.err != hipSuccess) return hip_fail(h, dg.err, "hipSetDevice");
    const size_t N = h->cfg.N, b = (size_t)B, nx = b * (N + 1) * 6, nu = b * N * 2;
    Stager st;
    const double *d_x, *d_u, *d_dual, *d_xref, *d_uref, *d_w, *d_gx, *d_gu;
    const int* d_st;
    tt_track_vjp_bounds_out dout;
    st.in(x, nx, &d_x);
    st.in(u, nu, &d_u);
    st.in(dual, b * (N + 1) * ttmpc::kDualPerStage, &d_dual);
    st.in(xref, nx, &d_xref);
    st.in(uref, nu, &d_uref);
    st.in(wq_wr, b * 8, &d_w);
    st.in(grad_x, nx, &d_gx);
    st.in(grad_u, nu, &d_gu);
    st.in(status, b, &d_st);
    st.out(out->g_x0, b * 6, &dout.g_x0);
    st.out(out->g_xref, nx, &dout.g_xref);
    st.out(out->g_uref, nu, &dout.g_uref);
    st.out(out->g_wq_wr, b * 8, &dout.g_wq_wr);
    st.out(out->vjp_status, b, &dout.vjp_status);
    if (accumulate) {
        st.inout(out->g_model, b * 3, &dout.g_model);
        st.inout(out->g_bounds, b * 16, &dout.g_bounds);
    } else {
        st.out(out->g_model, b * 3, &dout.g_model);
        st.out(out->g_bounds, b * 16, &dout.g_bounds);
    }
    if (!st.carve(h->xfer)) return no_memory(h, "adjoint staging");
    hipStream_t s = h->stream;
    return st.run(h, s, "adjoint", [&] {
        return tt_track_vjp_bounds_device(handle, B, d_x, d_u, d_dual, d_xref, d_uref, d_w, d_st, d_gx, d_gu, &dout,
                                          accumulate, s);
    });
}

int tt_track_vjp_model(void* handle, int B, const double* x, const double* u, const double* dual, const double* xref,
                       const double* uref, const double* wq_wr, const int* status, const double* grad_x,
                       const double* grad_u, const tt_track_vjp_model_out* out, int accumulate) {
    tt_track_vjp_bounds_out o;
    return tt_track_vjp_bounds(handle, B, x, u, dual, xref, uref, wq_wr, status, grad_x, grad_u, widen(out, o),
                               accumulate);
}

int tt_track_vjp(void* handle, int B, const double* x, const double* u, const double* dual, const double* xref,
                 const double* uref, const double* wq_wr, const int* status, const double* grad_x,
                 const double* grad_u, const tt_track_vjp_out* out) {
    tt_track_vjp_model_out o;
    return tt_track_vjp_model(handle, B, x, u, dual, xref, uref, wq_wr, status, grad_x, grad_u, widen(out, o), 0);
}

int tt_set_model(void* handle, double L1, double L2, double Mh) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return fail(nullptr, -EINVAL, "NULL handle%s");
    if (is_obca(h->cfg))
        return fail(h, -EINVAL, "the geometry of an OBCA handle also enters its H-representations: create a new handle%s");
    if (!(L1 > 0) || !(L2 > 0) || !isfinite(L1) || !isfinite(L2) || !isfinite(Mh))
        return fail(h, -EINVAL, "params L1, L2 must be > 0 and M finite%s");
    // every launch path fills its kernel arguments from cfg (fill_model): nothing on the device holds the old values
    h->cfg.L1 = L1;
    h->cfg.L2 = L2;
    h->cfg.Mh = Mh;
    return 0;
}

int tt_get_model(void* handle, double* L1, double* L2, double* Mh) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return fail(nullptr, -EINVAL, "NULL handle%s");
    if (L1) *L1 = h->cfg.L1;
    if (L2) *L2 = h->cfg.L2;
    if (Mh) *Mh = h->cfg.Mh;
    return 0;
}

int tt_set_bounds(void* handle, const double* xlb, const double* xub, const double* ulb, const double* uub) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return fail(nullptr, -EINVAL, "NULL handle%s");
    if (is_obca(h->cfg))
        return fail(h, -EINVAL, "tt_set_bounds changes the box of a tracking handle; an OBCA handle keeps the box it was "
                                "created with%s");
    if (!xlb || !xub || !ulb || !uub) return fail(h, -EINVAL, "NULL argument%s");
    for (int i = 0; i < 6; ++i)  // (a NaN fails the comparison, as in tt_create)
        if (!(xlb[i] <= xub[i])) return fail(h, -EINVAL, "state bound lb > ub%s");
    for (int i = 0; i < 2; ++i)
        if (!(ulb[i] <= uub[i])) return fail(h, -EINVAL, "input bound lb > ub%s");
    // every launch path copies the box into its kernel arguments (fill_model) and launch_track picks its build from
    // the bound pattern of those arguments: nothing on the device, and no choice made at tt_create, holds the old box
    memcpy(h->xlb, xlb, sizeof h->xlb);
    memcpy(h->xub, xub, sizeof h->xub);
    memcpy(h->ulb, ulb, sizeof h->ulb);
    memcpy(h->uub, uub, sizeof h->uub);
    return 0;
}

int tt_get_bounds(void* handle, double* xlb, double* xub, double* ulb, double* uub) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return fail(nullptr, -EINVAL, "NULL handle%s");
    if (is_obca(h->cfg)) return fail(h, -EINVAL, "tt_get_bounds reads the box of a tracking handle%s");
    if (xlb) memcpy(xlb, h->xlb, sizeof h->xlb);
    if (xub) memcpy(xub, h->xub, sizeof h->xub);
    if (ulb) memcpy(ulb, h->ulb, sizeof h->ulb);
    if (uub) memcpy(uub, h->uub, sizeof h->uub);
    return 0;
}

long long tt_track_dual_len(int N) { return N < 1 ? -EINVAL : (long long)ttmpc::kDualPerStage * (N + 1); }

#ifdef TT_STAMPS
// Diagnostic-build-only entry point: per-instance phase cycle sums into d_stamps[B][kNumPhases].
int ttx_solve_stamped(void* handle, int B, const double* d_x0, const double* d_xref, const double* d_uref,
                      double* d_x_out, double* d_u_out, int* d_status, int* d_iters, unsigned long long* d_stamps,
                      void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || B <= 0 || !d_stamps) return -EINVAL;
    ttmpc::TrackArgs a;
    if (const int rc = make_track_args(h, B, a)) return rc;
    a.x0 = d_x0;
    a.xref = d_xref;
    a.uref = d_uref;
    a.xout = d_x_out;
    a.uout = d_u_out;
    a.status = d_status;
    a.iters = d_iters;
    a.stamps = d_stamps;
    hipError_t e = ttmpc::launch_track(a, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? 0 : hip_fail(h, e, "stamped launch");
}
#endif

// both device entries of the OBCA solve: d_obs [B][M][4] / d_dmin [B] are the per-instance scenes (nullptr: the handle's)
static int obca_solve_device(void* handle, int B, const double* d_x0, const double* d_xgoal, const double* d_xref,
                             const double* d_uref, const double* d_z_guess, double* d_x_out, double* d_u_out,
                             double* d_z_out, int* d_status, int* d_iters, double* d_kkt_res, double* d_iterate_out,
                             const double* d_obs, const double* d_dmin, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, B, kHandle | kObcaOnly | kSign | kEmpty | kRange, nullptr, 1 << 24)) return result(rc);
    const bool plan = h->cfg.variant == TT_VARIANT_OBCA_PLAN;
    if (!d_x0 || !d_x_out || !d_u_out || !d_status) return fail(h, -EINVAL, "NULL device buffer%s");
    if (plan && !d_xgoal) return fail(h, -EINVAL, "plan variant needs the goal states%s");
    if (!plan && (!d_xref || !d_uref)) return fail(h, -EINVAL, "MPC+OBCA variant needs reference states/inputs%s");
    DeviceGuard dg(h->device);
    hipError_t e = dg.err;
    if (e != hipSuccess) return hip_fail(h, e, "hipSetDevice");
    const size_t board_bytes = ((size_t)B + 1) * ttmpc::kObcaBoardStride * 8;
    if (!h->ows.ensure((size_t)B * ttmpc::obca_ws_doubles(h->cfg.N, h->cfg.M) * 8) || !h->board.ensure(board_bytes))
        return fail(h, -ENOMEM, "OBCA workspace allocation failed for B=%s", std::to_string(B).c_str());
    ttmpc::ObcaArgs a;
    memset(&a, 0, sizeof a);
    a.N = h->cfg.N;
    a.M = h->cfg.M;
    a.B = B;
    a.mode = plan ? ttmpc::OBCA_PLAN : ttmpc::OBCA_TRACK;
    a.max_iter = h->cfg.max_iter;
    a.acc_iter = h->cfg.acc_iter;
    a.dual_init = h->cfg.dual_init;
    a.W1 = h->cfg.W1;
    a.W2 = h->cfg.W2;
    a.tol = h->cfg.tol;
    a.acc_tol = h->cfg.acc_tol;
    a.dmin = h->dmin;
    a.eq_tol = 1e-5;   // trajectory_optimization.py:136-139
    a.fin_tol = 1e-2;  // trajectory_optimization.py:172-173
    a.tfac = plan ? 100.0 : 1.0;  // trajectory_optimization.py:180 / mpc_control_obs.py:39
    fill_model(a, h);
    memcpy(a.obs, h->obs, sizeof a.obs);
    a.obs_b = d_obs;
    a.dmin_b = d_dmin;
    a.x0 = d_x0;
    a.xgoal = d_xgoal;
    a.xref = d_xref;
    a.uref = d_uref;
    a.zg = d_z_guess;
    a.xout = d_x_out;
    a.uout = d_u_out;
    a.zout = d_z_out;
    a.status = d_status;
    a.iters = d_iters;
    a.kkt = d_kkt_res;
    a.itout = d_iterate_out;
    a.ws = static_cast<double*>(h->ows.p);
    a.stamps = h->obca_stamps;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (h->nhelp < 0) {  // one helper workgroup per CU: they run while CUs are idle (the batch's tail)
        int cus = 0;
        e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device);
        if (e != hipSuccess) return hip_fail(h, e, "hipDeviceGetAttribute");
        h->nhelp = cus;
    }
    a.board = static_cast<unsigned long long*>(h->board.p);
    a.nhelp = h->nhelp;
    a.spin_ticks = h->spin_ticks;
    a.fail_b = h->fail_b;
    e = hipMemsetAsync(a.board, 0, board_bytes, s);
    if (e != hipSuccess) return hip_fail(h, e, "hipMemsetAsync (OBCA board)");
    e = ttmpc::launch_obca(a, s);
    if (e != hipSuccess) return hip_fail(h, e, "OBCA kernel launch");
    return 0;
}

int tt_obca_solve_batch_iterate_device(void* handle, int B, const double* d_x0, const double* d_xgoal,
                                       const double* d_xref, const double* d_uref, const double* d_z_guess,
                                       double* d_x_out, double* d_u_out, double* d_z_out, int* d_status, int* d_iters,
                                       double* d_kkt_res, double* d_iterate_out, void* stream) {
    return obca_solve_device(handle, B, d_x0, d_xgoal, d_xref, d_uref, d_z_guess, d_x_out, d_u_out, d_z_out, d_status,
                             d_iters, d_kkt_res, d_iterate_out, nullptr, nullptr, stream);
}

int tt_obca_solve_batch_scenes_device(void* handle, int B, const double* d_x0, const double* d_xgoal,
                                      const double* d_xref, const double* d_uref, const double* d_z_guess,
                                      double* d_x_out, double* d_u_out, double* d_z_out, int* d_status, int* d_iters,
                                      double* d_kkt_res, double* d_iterate_out, const tt_obca_scenes* d_scenes,
                                      void* stream) {
    return obca_solve_device(handle, B, d_x0, d_xgoal, d_xref, d_uref, d_z_guess, d_x_out, d_u_out, d_z_out, d_status,
                             d_iters, d_kkt_res, d_iterate_out, d_scenes ? d_scenes->obstacles : nullptr,
                             d_scenes ? d_scenes->d_min : nullptr, stream);
}

int tt_obca_solve_batch_device(void* handle, int B, const double* d_x0, const double* d_xgoal, const double* d_xref,
                               const double* d_uref, const double* d_z_guess, double* d_x_out, double* d_u_out,
                               double* d_z_out, int* d_status, int* d_iters, double* d_kkt_res, void* stream) {
    return tt_obca_solve_batch_iterate_device(handle, B, d_x0, d_xgoal, d_xref, d_uref, d_z_guess, d_x_out, d_u_out,
                                              d_z_out, d_status, d_iters, d_kkt_res, nullptr, stream);
}

// tt_set_scene's rule, for B scenes at once (either array may be nullptr)
static int check_scenes(Handle* h, int B, const double* obstacles, const double* d_min) {
    const size_t M = h->cfg.M;
    for (size_t i = 0; obstacles && i < (size_t)B * M; ++i) {
        const double* o = obstacles + 4 * i;
        if (!isfinite(o[0]) || !isfinite(o[1]) || !isfinite(o[2]) || !isfinite(o[3]) || !(o[2] > 0) || !(o[3] > 0))
            return fail(h, -EINVAL, "obstacles must be finite with w, h > 0 (instance %s)", std::to_string(i / M).c_str());
    }
    for (int b = 0; d_min && b < B; ++b)
        if (!isfinite(d_min[b]) || d_min[b] < 0)
            return fail(h, -EINVAL, "d_min must be finite and >= 0 (instance %s)", std::to_string(b).c_str());
    return 0;
}

// both host entries of the OBCA solve (sc nullptr: the handle's scene)
static int obca_solve_host(void* handle, int B, const double* x0, const double* xgoal, const double* xref,
                           const double* uref, const double* z_guess, double* x_out, double* u_out, double* z_out,
                           int* status, int* iters, double* kkt_res, double* iterate_out, const tt_obca_scenes* sc) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, B, kHandle | kObcaOnly | kSign | kEmpty)) return result(rc);
    const double* obs = sc ? sc->obstacles : nullptr;
    const double* dmin = sc ? sc->d_min : nullptr;
    if (const int rc = check_scenes(h, B, obs, dmin)) return rc;  // (nothing staged, nothing launched)
    const bool plan = h->cfg.variant == TT_VARIANT_OBCA_PLAN;
    if (!x0 || !status || (plan && !xgoal) || (!plan && (!xref || !uref)))
        return fail(h, -EINVAL, "NULL host buffer%s");
    DeviceGuard dg(h->device);
    if (dg.err != hipSuccess) return hip_fail(h, dg.err, "hipSetDevice");
    const size_t N = h->cfg.N, nz = ttmpc::obca_n(h->cfg.N, h->cfg.M), b = (size_t)B;
    // the launch writes X, U, status, iters and kkt whether or not the caller wants them back
    Stager st;
    const double *d_x0, *d_xg, *d_xr, *d_ur, *d_zg, *d_obs, *d_dmin;
    double *d_xo, *d_uo, *d_zo, *d_kkt, *d_itout;
    int *d_st, *d_it;
    st.in(obs, b * 4 * h->cfg.M, &d_obs);
    st.in(dmin, b, &d_dmin);
    st.in(x0, b * 6, &d_x0);
    st.in(plan ? xgoal : nullptr, b * 6, &d_xg);
    st.in(plan ? nullptr : xref, b * (N + 1) * 6, &d_xr);
    st.in(plan ? nullptr : uref, b * N * 2, &d_ur);
    st.in(z_guess, b * nz, &d_zg);
    st.out(iterate_out, b * ttmpc::obca_iterate_len(h->cfg.N, h->cfg.M), &d_itout);  // (the diagnostic export)
    st.out(x_out, b * (N + 1) * 6, &d_xo, true);
    st.out(u_out, b * N * 2, &d_uo, true);
    st.out(z_out, b * nz, &d_zo);
    st.out(status, b, &d_st, true);
    st.out(iters, b, &d_it, true);
    st.out(kkt_res, b, &d_kkt, true);
    if (!st.carve(h->xfer))
        return fail(h, -ENOMEM, "device workspace allocation failed for B=%s", std::to_string(B).c_str());
    hipStream_t s = h->stream;
    return st.run(h, s, "OBCA solve", [&] {
        return obca_solve_device(h, B, d_x0, d_xg, d_xr, d_ur, d_zg, d_xo, d_uo, d_zo, d_st, d_it, d_kkt, d_itout, d_obs,
                                 d_dmin, s);
    });
}

int tt_obca_solve_batch_iterate(void* handle, int B, const double* x0, const double* xgoal, const double* xref,
                                const double* uref, const double* z_guess, double* x_out, double* u_out, double* z_out,
                                int* status, int* iters, double* kkt_res, double* iterate_out) {
    return obca_solve_host(handle, B, x0, xgoal, xref, uref, z_guess, x_out, u_out, z_out, status, iters, kkt_res,
                           iterate_out, nullptr);
}

int tt_obca_solve_batch_scenes(void* handle, int B, const double* x0, const double* xgoal, const double* xref,
                               const double* uref, const double* z_guess, double* x_out, double* u_out, double* z_out,
                               int* status, int* iters, double* kkt_res, double* iterate_out,
                               const tt_obca_scenes* scenes) {
    return obca_solve_host(handle, B, x0, xgoal, xref, uref, z_guess, x_out, u_out, z_out, status, iters, kkt_res,
                           iterate_out, scenes);
}

int tt_obca_solve_batch(void* handle, int B, const double* x0, const double* xgoal, const double* xref,
                        const double* uref, const double* z_guess, double* x_out, double* u_out, double* z_out,
                        int* status, int* iters, double* kkt_res) {
    return tt_obca_solve_batch_iterate(handle, B, x0, xgoal, xref, uref, z_guess, x_out, u_out, z_out, status, iters,
                                       kkt_res, nullptr);
}

// the MPC+OBCA adjoint keeps its whole record in LDS
static int obca_vjp_horizon(Handle* h) {
    if (h->cfg.N <= ttmpc::obca_vjp_max_horizon()) return 0;
    return fail(h, -EINVAL, "the MPC+OBCA adjoint keeps its record in LDS: horizon must be <= %s",
                std::to_string(ttmpc::obca_vjp_max_horizon()).c_str());
}

long long tt_obca_vjp_params_work_bytes(int N, int M) {
    return (N < 1 || M < 1) ? -EINVAL : (long long)(8 * ttmpc::obca_vjp_params_work_doubles(N, M));
}

// The eight entries below run one device body and one host stager over the widest call, the geometry entries': each
// widens its out-struct to tt_obca_vjp_geometry_out and names the kernel instantiation (ttmpc::ObcaVjpKind) its own
// rule picks.  NULL stays NULL (the bodies' to refuse).
static const tt_obca_vjp_geometry_out* widen(const tt_obca_vjp_params_out* out, tt_obca_vjp_geometry_out& o) {
    if (!out) return nullptr;
    o = {out->g_x0, out->g_xref, out->g_uref, out->vjp_status, out->g_obstacles, out->g_dmin, out->g_Q, out->g_R,
         nullptr};
    return &o;
}

static const tt_obca_vjp_geometry_out* widen(const tt_obca_vjp_out* out, tt_obca_vjp_geometry_out& o) {
    if (!out) return nullptr;
    o = {out->g_x0, out->g_xref, out->g_uref, out->vjp_status, nullptr, nullptr, nullptr, nullptr, nullptr};
    return &o;
}

// tt_obca_vjp_scenes* / _geometry*: the geometry instantiation iff g_geometry is wanted; else the plain one (no work
// buffer) iff no parameter output is wanted and, in a device entry, no work buffer is given; else the params one
static ttmpc::ObcaVjpKind obca_vjp_kind(const tt_obca_vjp_geometry_out* o, const void* work) {
    if (o && o->g_geometry) return ttmpc::kObcaVjpGeom;
    const bool plain = o && !work && !o->g_obstacles && !o->g_dmin && !o->g_Q && !o->g_R;
    return plain ? ttmpc::kObcaVjpPlain : ttmpc::kObcaVjpParams;
}

// the checks the device body and the host stager share, in this order (nothing staged yet)
static int obca_vjp_checks(Handle* h, int B, const void* grad_x, const void* grad_u, const void* xref, const void* uref,
                           const tt_obca_vjp_geometry_out* out) {
    if (const int rc = prelude(h, B, kHandle | kObcaOnly | kNotPlan | kSign)) return rc;
    if (!grad_x && !grad_u) return fail(h, -EINVAL, "grad_x and grad_u are both NULL: no loss to differentiate%s");
    if (const int rc = obca_vjp_horizon(h)) return rc;
    if (out && ((out->g_Q && !xref) || (out->g_R && !uref)))
        return fail(h, -EINVAL, "g_Q needs xref and g_R needs uref%s");
    return 0;
}

// (d_obs [B][M][4]: per-instance obstacles, nullptr: the handle's; d_work: not read by the plain kind)
static int obca_vjp_device(void* handle, int B, const double* d_iterate, const int* d_status, const double* d_xref,
                           const double* d_uref, const double* d_grad_x, const double* d_grad_u,
                           const tt_obca_vjp_geometry_out* d_out, void* d_work, const double* d_obs,
                           ttmpc::ObcaVjpKind kind, void* stream) {
    Handle* h = static_cast<Handle*>(handle);
    const bool plain = kind == ttmpc::kObcaVjpPlain;
    if (const int rc = obca_vjp_checks(h, B, d_grad_x, d_grad_u, d_xref, d_uref, d_out)) return rc;
    if (!plain && !d_work) return fail(h, -EINVAL, "NULL work buffer (tt_obca_vjp_params_work_bytes per instance)%s");
    if (const int rc = prelude(h, B, kEmpty | kRange)) return result(rc);
    if (!d_iterate || !d_status || !d_out) return fail(h, -EINVAL, "NULL device buffer%s");
    DeviceGuard dg(h->device);
    if (dg.err != hipSuccess) return hip_fail(h, dg.err, "hipSetDevice");
    ttmpc::ObcaVjpGeomArgs a = diff_args<ttmpc::ObcaVjpGeomArgs>(h, B, nullptr, nullptr, nullptr, nullptr, d_status);
    a.M = h->cfg.M;
    a.W1 = h->cfg.W1;
    a.W2 = h->cfg.W2;
    a.eq_tol = 1e-5;  // trajectory_optimization.py:136-139, as the solve sets it
    memcpy(a.obs, h->obs, sizeof a.obs);
    a.obs_b = d_obs;
    a.iterate = d_iterate;
    a.gx = d_grad_x;
    a.gu = d_grad_u;
    a.g_x0 = d_out->g_x0;
    a.g_xref = d_out->g_xref;
    a.g_uref = d_out->g_uref;
    a.vjp_status = d_out->vjp_status;
    a.xref = d_xref;
    a.uref = d_uref;
    a.g_obs = d_out->g_obstacles;
    a.g_dmin = d_out->g_dmin;
    a.g_Q = d_out->g_Q;
    a.g_R = d_out->g_R;
    a.work = static_cast<double*>(d_work);
    a.g_geom = d_out->g_geometry;
    const hipError_t e = ttmpc::launch_obca_vjp(a, kind, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return hip_fail(h, e, plain ? "OBCA adjoint kernel launch" : "OBCA params adjoint kernel launch");
    return 0;
}

// (scenes nullptr: the handle's scene)
static int obca_vjp_host(void* handle, int B, const double* iterate, const int* status, const double* xref,
                         const double* uref, const double* grad_x, const double* grad_u,
                         const tt_obca_vjp_geometry_out* out, const tt_obca_scenes* scenes, ttmpc::ObcaVjpKind kind) {
    Handle* h = static_cast<Handle*>(handle);
    const double* obs = scenes ? scenes->obstacles : nullptr;
    const bool plain = kind == ttmpc::kObcaVjpPlain;
    // (the adjoint does not read d_min, but a scene the solve would have refused is refused here too)
    if (h && is_obca(h->cfg) && scenes && scenes->d_min)
        if (const int rc = check_scenes(h, B, nullptr, scenes->d_min)) return rc;
    if (const int rc = obca_vjp_checks(h, B, grad_x, grad_u, xref, uref, out)) return rc;
    if (const int rc = prelude(h, B, kEmpty | kRange)) return result(rc);
    if (!iterate || !status || !out) return fail(h, -EINVAL, "NULL host buffer%s");
    if (const int rc = check_scenes(h, B, obs, nullptr)) return rc;
    DeviceGuard dg(h->device);
    if (dg.err != hipSuccess) return hip_fail(h, dg.err, "hipSetDevice");
    const size_t N = h->cfg.N, M = h->cfg.M, b = (size_t)B, nx = b * (N + 1) * 6, nu = b * N * 2;
    Stager st;
    const double *d_it, *d_gx, *d_gu, *d_xr, *d_ur, *d_obs;
    const int* d_st;
    double* d_work = nullptr;
    tt_obca_vjp_geometry_out dout;
    st.in(obs, b * 4 * M, &d_obs);
    st.in(iterate, b * ttmpc::obca_iterate_len(h->cfg.N, h->cfg.M), &d_it);
    st.in(grad_x, nx, &d_gx);
    st.in(grad_u, nu, &d_gu);
    st.in(status, b, &d_st);
    st.in(out->g_Q ? xref : nullptr, nx, &d_xr);  // (read for g_Q / g_R only)
    st.in(out->g_R ? uref : nullptr, nu, &d_ur);
    st.out(out->g_x0, b * 6, &dout.g_x0);
    st.out(out->g_xref, nx, &dout.g_xref);
    st.out(out->g_uref, nu, &dout.g_uref);
    st.out(out->vjp_status, b, &dout.vjp_status);
    st.out(out->g_obstacles, b * M * 4, &dout.g_obstacles);
    st.out(out->g_dmin, b, &dout.g_dmin);
    st.out(out->g_Q, b * 36, &dout.g_Q);
    st.out(out->g_R, b * 4, &dout.g_R);
    st.out(out->g_geometry, b * 5, &dout.g_geometry);
    if (!plain) st.out((double*)nullptr, b * ttmpc::obca_vjp_params_work_doubles(h->cfg.N, h->cfg.M), &d_work, true);
    if (!st.carve(h->xfer)) return no_memory(h, "adjoint staging");
    hipStream_t s = h->stream;
    return st.run(h, s, plain ? "OBCA adjoint" : "OBCA params adjoint", [&] {
        return obca_vjp_device(handle, B, d_it, d_st, d_xr, d_ur, d_gx, d_gu, &dout, d_work, d_obs, kind, s);
    });
}

int tt_obca_vjp_device(void* handle, int B, const double* d_iterate, const int* d_status, const double* d_grad_x,
                       const double* d_grad_u, const tt_obca_vjp_out* d_out, void* stream) {
    tt_obca_vjp_geometry_out o;
    return obca_vjp_device(handle, B, d_iterate, d_status, nullptr, nullptr, d_grad_x, d_grad_u, widen(d_out, o),
                           nullptr, nullptr, ttmpc::kObcaVjpPlain, stream);
}

int tt_obca_vjp(void* handle, int B, const double* iterate, const int* status, const double* grad_x,
                const double* grad_u, const tt_obca_vjp_out* out) {
    tt_obca_vjp_geometry_out o;
    return obca_vjp_host(handle, B, iterate, status, nullptr, nullptr, grad_x, grad_u, widen(out, o), nullptr,
                         ttmpc::kObcaVjpPlain);
}

int tt_obca_vjp_params_device(void* handle, int B, const double* d_iterate, const int* d_status, const double* d_xref,
                              const double* d_uref, const double* d_grad_x, const double* d_grad_u,
                              const tt_obca_vjp_params_out* d_out, void* d_work, void* stream) {
    tt_obca_vjp_geometry_out o;
    return obca_vjp_device(handle, B, d_iterate, d_status, d_xref, d_uref, d_grad_x, d_grad_u, widen(d_out, o), d_work,
                           nullptr, ttmpc::kObcaVjpParams, stream);
}

int tt_obca_vjp_params(void* handle, int B, const double* iterate, const int* status, const double* xref,
                       const double* uref, const double* grad_x, const double* grad_u,
                       const tt_obca_vjp_params_out* out) {
    tt_obca_vjp_geometry_out o;
    return obca_vjp_host(handle, B, iterate, status, xref, uref, grad_x, grad_u, widen(out, o), nullptr,
                         ttmpc::kObcaVjpParams);
}

int tt_obca_vjp_scenes_device(void* handle, int B, const double* d_iterate, const int* d_status, const double* d_xref,
                              const double* d_uref, const double* d_grad_x, const double* d_grad_u,
                              const tt_obca_vjp_params_out* d_out, void* d_work, const tt_obca_scenes* d_scenes,
                              void* stream) {
    tt_obca_vjp_geometry_out o;
    return tt_obca_vjp_geometry_device(handle, B, d_iterate, d_status, d_xref, d_uref, d_grad_x, d_grad_u,
                                       widen(d_out, o), d_work, d_scenes, stream);
}

int tt_obca_vjp_scenes(void* handle, int B, const double* iterate, const int* status, const double* xref,
                       const double* uref, const double* grad_x, const double* grad_u,
                       const tt_obca_vjp_params_out* out, const tt_obca_scenes* scenes) {
    tt_obca_vjp_geometry_out o;
    return tt_obca_vjp_geometry(handle, B, iterate, status, xref, uref, grad_x, grad_u, widen(out, o), scenes);
}

int tt_obca_vjp_geometry_device(void* handle, int B, const double* d_iterate, const int* d_status,
                                const double* d_xref, const double* d_uref, const double* d_grad_x,
                                const double* d_grad_u, const tt_obca_vjp_geometry_out* d_out, void* d_work,
                                const tt_obca_scenes* d_scenes, void* stream) {
    return obca_vjp_device(handle, B, d_iterate, d_status, d_xref, d_uref, d_grad_x, d_grad_u, d_out, d_work,
                           d_scenes ? d_scenes->obstacles : nullptr, obca_vjp_kind(d_out, d_work), stream);
}

int tt_obca_vjp_geometry(void* handle, int B, const double* iterate, const int* status, const double* xref,
                         const double* uref, const double* grad_x, const double* grad_u,
                         const tt_obca_vjp_geometry_out* out, const tt_obca_scenes* scenes) {
    return obca_vjp_host(handle, B, iterate, status, xref, uref, grad_x, grad_u, out, scenes,
                         obca_vjp_kind(out, nullptr));
}

int tt_set_geometry(void* handle, double L1, double L2, double Mh, double W1, double W2) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, 0, kHandle | kObcaOnly)) return rc;
    if (!(L1 > 0) || !(L2 > 0) || !(W1 > 0) || !(W2 > 0) || !isfinite(L1) || !isfinite(L2) || !isfinite(W1) ||
        !isfinite(W2) || !isfinite(Mh))
        return fail(h, -EINVAL, "params L1, L2, W1, W2 must be finite and > 0 and M finite%s");
    // every launch fills its kernel arguments from cfg: nothing on the device holds the old values
    h->cfg.L1 = L1;
    h->cfg.L2 = L2;
    h->cfg.Mh = Mh;
    h->cfg.W1 = W1;
    h->cfg.W2 = W2;
    return 0;
}

int tt_get_geometry(void* handle, double* L1, double* L2, double* Mh, double* W1, double* W2) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, 0, kHandle | kObcaOnly)) return rc;
    if (L1) *L1 = h->cfg.L1;
    if (L2) *L2 = h->cfg.L2;
    if (Mh) *Mh = h->cfg.Mh;
    if (W1) *W1 = h->cfg.W1;
    if (W2) *W2 = h->cfg.W2;
    return 0;
}

int tt_set_scene(void* handle, const double* obstacles, const double* d_min) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, 0, kHandle | kObcaOnly)) return rc;
    const int M = h->cfg.M;
    if (obstacles)
        for (int m = 0; m < M; ++m) {
            const double* o = obstacles + 4 * m;
            if (!isfinite(o[0]) || !isfinite(o[1]) || !isfinite(o[2]) || !isfinite(o[3]) || !(o[2] > 0) || !(o[3] > 0))
                return fail(h, -EINVAL, "obstacles must be finite with w, h > 0%s");
        }
    if (d_min && (!isfinite(*d_min) || *d_min < 0)) return fail(h, -EINVAL, "d_min must be finite and >= 0%s");
    // every launch fills its kernel arguments from the handle: nothing on the device holds the old scene
    if (obstacles) memcpy(h->obs, obstacles, sizeof(double) * 4 * M);
    if (d_min) h->dmin = *d_min;
    return 0;
}

int tt_get_scene(void* handle, double* obstacles, double* d_min) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, 0, kHandle | kObcaOnly)) return rc;
    if (obstacles) memcpy(obstacles, h->obs, sizeof(double) * 4 * h->cfg.M);
    if (d_min) *d_min = h->dmin;
    return 0;
}

/* diagnostics only (not part of include/ttmpc.h): per-instance phase cycle sums of the handle's next OBCA
 * launches into d_stamps[B][kObcaPhases] (device pointer; NULL switches it off).  Returns the phase count. */
int ttx_obca_set_stamps(void* handle, unsigned long long* d_stamps) {
    Handle* h = static_cast<Handle*>(handle);
    if (h) h->obca_stamps = d_stamps;
    return ttmpc::kObcaPhases;
}

/* diagnostics only: helper workgroups of the handle's OBCA launches (0: none, every instance runs its own block
 * passes; -1: one per CU, the default).  The results are bitwise the same either way (tests/test_gpu_obca.py). */
int ttx_obca_set_helpers(void* handle, int n) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return -EINVAL;
    h->nhelp = n < 0 ? -1 : n;
    return 0;
}

/* diagnostics only: the helper hand-off's spin limit in microseconds (0: the default 5 s) and one instance whose
 * hand-offs never complete (-1: none), so that it ends with TT_HANDOFF_TIMEOUT while its neighbours solve normally
 * (tests/test_gpu_obca.py::test_helper_handoff_timeout_is_reported_and_isolated). */
int ttx_obca_set_handoff_debug(void* handle, long long spin_us, int fail_b) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h || spin_us < 0) return -EINVAL;
    h->spin_ticks = (unsigned long long)spin_us * 100ull;  // s_memrealtime: 100 MHz
    h->fail_b = fail_b < 0 ? -1 : fail_b;
    return 0;
}
static_assert(TT_HANDOFF_TIMEOUT == 6, "tt_obca.hip kStatusHandoffTimeout");

int tt_plan_batch(void* handle, int B, const double* x0, const double* xgoal, const double* z_guess, double* x_out,
                  double* u_out, int* status, int* iters) {
    Handle* h = static_cast<Handle*>(handle);
    if (const int rc = prelude(h, B, kHandle | kPlanOnly)) return rc;
    if (!x_out || !u_out) return fail(h, -EINVAL, "NULL host buffer%s");
    return tt_obca_solve_batch(handle, B, x0, xgoal, nullptr, nullptr, z_guess, x_out, u_out, nullptr, status, iters,
                               nullptr);
}

void tt_destroy(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    if (!h) return;
    DeviceGuard dg(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    free_stage(h);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;  // (its device buffers go with it, under the handle's device)
}

const char* tt_last_error(void* handle) {
    Handle* h = static_cast<Handle*>(handle);
    return h ? h->err.c_str() : g_err.c_str();
}

int tt_lds_bytes(int N) { return ttmpc::lds_bytes(N); }
int tt_max_horizon(void) { return ttmpc::max_horizon(); }
const char* tt_version(void) { return "ttmpc 0.2 (gfx950: wave-per-instance Riccati IPM; workgroup-per-instance OBCA IPM)"; }
long long tt_obca_n(int N, int M) { return (N < 1 || M < 1) ? -EINVAL : (long long)ttmpc::obca_n(N, M); }
long long tt_obca_iterate_len(int N, int M) {
    return (N < 1 || M < 1) ? -EINVAL : (long long)ttmpc::obca_iterate_len(N, M);
}
long long tt_obca_workspace_bytes(int N, int M) {
    return (N < 1 || M < 1) ? -EINVAL : (long long)(8 * ttmpc::obca_ws_doubles(N, M));
}

}  // extern "C"
