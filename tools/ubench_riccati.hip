// Microbenchmark (diagnostic, never shipped): cycles per stage of the tracking kernel's Riccati stage
// loop (tt_track.hip phase_riccati, N = 20 unrolled) and of variants that drop or reshape one
// ingredient, to find what sets the per-stage latency.  One wave per workgroup (one wave per SIMD, as C2).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Icar-trailer-mpc_amd/csrc \
//         tools/ubench_riccati.hip -o tools/ubench_riccati && tools/ubench_riccati
#include "../car-trailer-mpc_amd/csrc/tt_track.hip"

#include <cstdio>
#include <algorithm>
#include <cmath>
#include <vector>

namespace ttmpc {
namespace {

constexpr int UB_BM = kMaskMPC | kDiagBit;
constexpr int UB_N = 20;
constexpr int UB_SR2 = 118;  // LDS image stride of the synthetic records (>= SR)

// Round 6: the shipped phase_riccati runs the input-shift form (four-term sums, tt_track.hip gu_shift).  V = 9 is that
// kernel; V = 50 is a private copy of round 5's stage (six-term sums, g_u in the affine slots) for the A/B in one
// binary; V = 51 is round 5's stage without the next-stage prefetch and the factor-row store (its floor).  The
// earlier variants (prefetch splits, paired reads, DPP P rows, bpermute PA columns, folded H_uu diagonals, the
// adjugate M) are recorded in DESIGN.md and profiles/r06/ubench_riccati_r5variants.txt; git history holds their code.
struct R5Map {
    int dj[6], di[6];
    int hs, ps;
    int gj0, gj1, gi0, gi1;
    double q2, dg;
    __device__ __forceinline__ static int dslot(int m, int n) {
        return (m < 6 && n < 6 && d_idx(m, n) >= 0) ? rAJ + d_idx(m, n) : (m < 6 && n == 6) ? rBH + m : PAD;
    }
    __device__ __forceinline__ void init(int i, int j, const double* QW) {
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            dj[m] = dslot(m, j);
            di[m] = dslot(m, i);
        }
        const int gi = (i < 6 && j == 6) ? i : (i == 6 && j < 6) ? j : -1;
        hs = (i == j && i < 6) ? rHD + i : (i < 6 && j < 6 && w_idx(i, j) >= 0) ? rWC + w_idx(i, j)
           : gi >= 0 ? rGF + gi : PAD;
        q2 = (i < 6 && j < 6) ? 2.0 * QW[i * 6 + j] : 0.0;
        dg = (i == j && i < 6) ? 1.0 : 0.0;
        ps = (i <= j && j < 6) ? rPS + sym_idx(i, j) : (i < 6 && j == 6) ? rPV + i : -1;
        gj0 = j == 6 ? rGF + 6 : PAD;
        gj1 = j == 6 ? rGF + 7 : PAD;
        gi0 = i == 6 ? rGF + 6 : PAD;
        gi1 = i == 6 ? rGF + 7 : PAD;
    }
};
struct R5Ops {
    double dj[6], di[6], h, sgu0, sgu1, gj0, gj1, gi0, gi1;
};
__device__ __forceinline__ void r5_ops_a(const Ctx<UB_BM>& c, const R5Map& m, int k, R5Ops& o) {
#pragma unroll
    for (int t = 0; t < 6; ++t) o.dj[t] = c.r(m.dj[t], k);
    o.sgu0 = c.r(rSGU, k);
    o.sgu1 = c.r(rSGU + 1, k);
}
__device__ __forceinline__ void r5_ops_b(const Ctx<UB_BM>& c, const R5Map& m, int k, double dw, R5Ops& o) {
#pragma unroll
    for (int t = 0; t < 6; ++t) o.di[t] = c.r(m.di[t], k);
    o.h = m.q2 + m.dg * dw + c.r(m.hs, k);
    o.gj0 = c.r(m.gj0, k);
    o.gj1 = c.r(m.gj1, k);
    o.gi0 = c.r(m.gi0, k);
    o.gi1 = c.r(m.gi1, k);
}

// Round 8: private copies of the shipped four-term stage, for the A/B of its schedule in one binary (results and what
// shipped: DESIGN.md section 3, profiles/r08_riccati_reads/).  V = 60 is the stage as round 7 shipped it, V = 66 the stage
// as phase_riccati has it now (PAF alone).
//   PIN   = false: no fence behind the second prefetch half, which the compiler then sinks below the F, G, M arithmetic
//           to just ahead of the P^ write; true: fenced there, and the last subtraction and the P^ write fenced off too
//   GSEL  = g_u' as one wave-uniform b128 read and four selects instead of four reads that return the zero pad to most lanes
//   DEFER = the factor-row store of stage k issued one stage later, behind the first prefetch half of stage k - 1
//   PAF   = PA and its tile write first, the H_uu inverse (det, rcp, two Newton steps) behind the tile reads
//   AF    = the fences around the first prefetch half (false: the compiler places it); AB = both halves behind the PA reads
template <bool PIN, bool GSEL, bool DEFER, bool PAF, bool AF = true, bool AB = false>
__device__ __forceinline__ bool ub_sweep4(const Ctx<UB_BM>& c, double dw) {
    constexpr int NS = UB_N;
    const int N = c.N, i = c.lane >> 3, j = c.lane & 7;
    EpMap m;
    m.init(i, j, c.sm + hQW);
    const double dt = c.dt, dt2 = dt * dt;
    const double r00 = 2.0 * c.h(hRW), r01 = 2.0 * c.h(hRW + 1), r11 = 2.0 * c.h(hRW + 3);
    double* PF = c.sm + hPF;
    double* PT = c.sm + hPT;
    const int sw_i = i & 4, sw_j = j & 4;
    const int pf_own = 8 * i + (j ^ sw_i);
    const double hb = m.q2 + m.dg * dw;
    double Pij = hb + c.rl(m.hs, N);
    PF[pf_own] = Pij;
    asm volatile("" ::: "memory");
    pstore(c, m.ps >= 0, m.ps, N, Pij);
    bool pd = true;
    const bool own_p = m.ps >= 0;
    const bool k_row = i >= 6 && j < 7;
    const int st_row = own_p ? m.ps : k_row ? (j < 6 ? rK + 6 * (i - 6) + j : rKF + (i - 6)) : rDX + 7;
    double sv = 0.0;  // DEFER: the store value of the stage before
    struct Ops {
        double dj[4], di[4], h, sgu0, sgu1, gj0, gj1, gi0, gi1;
        double2 gu;
    };
    auto ops_a = [&](int k, Ops& o) {
#pragma unroll
        for (int t = 0; t < 4; ++t) o.dj[t] = c.rl(m.dj[t], k);
        o.sgu0 = c.r(rSGU, k);
        o.sgu1 = c.r(rSGU + 1, k);
    };
    auto ops_b = [&](int k, Ops& o) {
#pragma unroll
        for (int t = 0; t < 4; ++t) o.di[t] = c.rl(m.di[t], k);
        o.h = c.rl(m.hs, k);
        if constexpr (GSEL) {
            o.gu = ld2(&c.rl(rGU, k));
        } else {
            o.gj0 = c.rl(m.gj0, k);
            o.gj1 = c.rl(m.gj1, k);
            o.gi0 = c.rl(m.gi0, k);
            o.gi1 = c.rl(m.gi1, k);
        }
    };
    auto stage = [&](int k, const Ops& o, Ops& nx, int kn) {
        const double2 r01v = ld2(PF + 8 * i + sw_i), r23v = ld2(PF + 8 * i + (2 ^ sw_i));
        const double2 p5 = ld2(PF + 40);
        const double p44 = PF[32];
        if constexpr (AF) __builtin_amdgcn_sched_barrier(0);
        if constexpr (!AB) ops_a(kn, nx);
        if constexpr (DEFER) {
            if (k < NS - 1) c.r(st_row, k + 1) = sv;
        }
        if constexpr (AF) __builtin_amdgcn_sched_barrier(0);
        double i00, i01, i11;
        auto huu = [&]() {
            const double h00 = r00 + o.sgu0 + dw + dt2 * p5.y, h01 = r01 + dt2 * p5.x, h11 = r11 + o.sgu1 + dw + dt2 * p44;
            const double det = h00 * h11 - h01 * h01;
            pd = pd & (h00 > 0.0) & (h11 > 0.0) & (det > 1e-13 * h00 * h11);
            const double id = frcp(det);
            i00 = h11 * id, i01 = -h01 * id, i11 = h00 * id;
        };
        if constexpr (!PAF) huu();
        double pa = fma(r01v.x, o.dj[0], Pij), pb = r01v.y * o.dj[1];
        pa = fma(r23v.x, o.dj[2], pa);
        pb = fma(r23v.y, o.dj[3], pb);
        const double PAij = pa + pb;
        PT[8 * j + (i ^ sw_j)] = PAij;
        asm volatile("" ::: "memory");
        const double2 c01 = ld2(PT + 8 * j + sw_j), c23 = ld2(PT + 8 * j + (2 ^ sw_j)), c45 = ld2(PT + 8 * j + (4 ^ sw_j));
        const double2 gi = ld2(PT + 8 * i + (4 ^ sw_i));
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (AB) ops_a(kn, nx);
        ops_b(kn, nx);
        if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
        if constexpr (PAF) huu();  // H_uu^-1 in the shadow of the PA tile's round trip, not ahead of its write
        double gj0, gj1, gi0, gi1;
        if constexpr (GSEL) {
            gj0 = j == 6 ? o.gu.x : 0.0;
            gj1 = j == 6 ? o.gu.y : 0.0;
            gi0 = i == 6 ? o.gu.x : 0.0;
            gi1 = i == 6 ? o.gu.y : 0.0;
        } else {
            gj0 = o.gj0, gj1 = o.gj1, gi0 = o.gi0, gi1 = o.gi1;
        }
        double fa = fma(o.di[0], c01.x, PAij + (hb + o.h)), fb = o.di[1] * c01.y;
        fa = fma(o.di[2], c23.x, fa);
        fb = fma(o.di[3], c23.y, fb);
        const double F = fa + fb;
        const double g0j = fma(dt, c45.y, gj0), g1j = fma(dt, c45.x, gj1);
        const double g0i = fma(dt, gi.y, gi0), g1i = fma(dt, gi.x, gi1);
        const double m0 = fma(i00, g0j, i01 * g1j), m1 = fma(i01, g0j, i11 * g1j);
        double kv = i == 6 ? -m0 : -m1;
        const double gm = fma(g0i, m0, g1i * m1);
        if constexpr (PIN) asm volatile("" : "+v"(kv));
        if constexpr (PIN) __builtin_amdgcn_sched_barrier(0);
        Pij = F - gm;
        PF[pf_own] = Pij;
        asm volatile("" ::: "memory");
        if constexpr (DEFER) sv = own_p ? Pij : kv;
        else c.r(st_row, k) = own_p ? Pij : kv;
    };
    Ops oa, ob;
    ops_a(N - 1, oa);
    ops_b(N - 1, oa);
#pragma unroll
    for (int k = NS - 1; k >= 1; k -= 2) {
        stage(k, oa, ob, k - 1);
        stage(k - 1, ob, oa, k >= 2 ? k - 2 : 0);
    }
    if constexpr (DEFER) c.r(st_row, 0) = sv;
    __syncthreads();
    return pd;
}

template <int V>
__device__ __forceinline__ bool ub_riccati(const Ctx<UB_BM>& c, double dw) {
    if constexpr (V == 9) {
        return phase_riccati<UB_BM, UB_N>(c, dw);
    } else if constexpr (V == 69) {
        return ub_sweep4<false, true, false, true>(c, dw);          // PA first, g select
    } else if constexpr (V == 70) {
        return ub_sweep4<false, false, false, true, false>(c, dw);  // PA first, first half unfenced
    } else if constexpr (V == 71) {
        return ub_sweep4<false, false, false, true, true, true>(c, dw);  // PA first, both halves behind the PA reads
    } else if constexpr (V >= 60) {
        // 60 round 7 | 61 fenced | 62 fenced, g select | 63 fenced, late store | 64 fenced, both
        // 65 late store | 66 PA first | 67 PA first, late store | 68 fenced, PA first, late store
        return ub_sweep4<(V >= 61 && V <= 64) || V == 68, (V == 62 || V == 64), (V == 63 || V == 64 || V == 65 || V >= 67),
                         (V >= 66)>(c, dw);
    } else {
        constexpr int NS = UB_N;
        constexpr bool full = V == 50;
        const int N = c.N, i = c.lane >> 3, j = c.lane & 7;
        R5Map m;
        m.init(i, j, c.sm + hQW);
        const double dt = c.dt, dt2 = dt * dt;
        const double r00 = 2.0 * c.h(hRW), r01 = 2.0 * c.h(hRW + 1), r11 = 2.0 * c.h(hRW + 3);
        double* PF = c.sm + hPF;
        double* PT = c.sm + hPT;
        const int sw_i = i & 4, sw_j = j & 4;
        const int pf_own = 8 * i + (j ^ sw_i);
        double Pij = m.q2 + m.dg * dw + c.r(m.hs, N);
        PF[pf_own] = Pij;
        asm volatile("" ::: "memory");
        bool pd = true;
        const bool own_p = m.ps >= 0;
        const bool k_row = i >= 6 && j < 7;
        const int st_row = own_p ? m.ps : k_row ? (j < 6 ? rK + 6 * (i - 6) + j : rKF + (i - 6)) : rDX + 7;
        auto stage = [&](int k, const R5Ops& o, R5Ops& nx, int kn) {
            const double2 r01v = ld2(PF + 8 * i + sw_i), r23v = ld2(PF + 8 * i + (2 ^ sw_i)), r45v = ld2(PF + 8 * i + (4 ^ sw_i));
            const double2 p5 = ld2(PF + 40);
            const double p44 = PF[32];
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (full) r5_ops_a(c, m, kn, nx);
            __builtin_amdgcn_sched_barrier(0);
            const double h00 = r00 + o.sgu0 + dw + dt2 * p5.y, h01 = r01 + dt2 * p5.x, h11 = r11 + o.sgu1 + dw + dt2 * p44;
            const double det = h00 * h11 - h01 * h01;
            pd = pd & (h00 > 0.0) & (h11 > 0.0) & (det > 1e-13 * h00 * h11);
            const double id = frcp(det), i00 = h11 * id, i01 = -h01 * id, i11 = h00 * id;
            double pa = fma(r01v.x, o.dj[0], Pij), pb = r01v.y * o.dj[1];
            pa = fma(r23v.x, o.dj[2], pa);
            pb = fma(r23v.y, o.dj[3], pb);
            pa = fma(r45v.x, o.dj[4], pa);
            pb = fma(r45v.y, o.dj[5], pb);
            const double PAij = pa + pb;
            PT[8 * j + (i ^ sw_j)] = PAij;
            asm volatile("" ::: "memory");
            const double2 c01 = ld2(PT + 8 * j + sw_j), c23 = ld2(PT + 8 * j + (2 ^ sw_j)), c45 = ld2(PT + 8 * j + (4 ^ sw_j));
            const double2 gi = ld2(PT + 8 * i + (4 ^ sw_i));
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (full) r5_ops_b(c, m, kn, dw, nx); else nx = o;
            double fa = fma(o.di[0], c01.x, PAij + o.h), fb = o.di[1] * c01.y;
            fa = fma(o.di[2], c23.x, fa);
            fb = fma(o.di[3], c23.y, fb);
            fa = fma(o.di[4], c45.x, fa);
            fb = fma(o.di[5], c45.y, fb);
            const double F = fa + fb;
            const double g0j = fma(dt, c45.y, o.gj0), g1j = fma(dt, c45.x, o.gj1);
            const double g0i = fma(dt, gi.y, o.gi0), g1i = fma(dt, gi.x, o.gi1);
            const double m0 = fma(i00, g0j, i01 * g1j), m1 = fma(i01, g0j, i11 * g1j);
            Pij = F - fma(g0i, m0, g1i * m1);
            PF[pf_own] = Pij;
            asm volatile("" ::: "memory");
            if constexpr (full) c.r(st_row, k) = own_p ? Pij : (i == 6 ? -m0 : -m1);
        };
        R5Ops oa, ob;
        r5_ops_a(c, m, N - 1, oa);
        r5_ops_b(c, m, N - 1, dw, oa);
#pragma unroll
        for (int k = NS - 1; k >= 1; k -= 2) {
            stage(k, oa, ob, k - 1);
            stage(k - 1, ob, oa, k >= 2 ? k - 2 : 0);
        }
        return pd;
    }
}

template <int V>
__global__ __launch_bounds__(64) void ub_kernel(int reps, unsigned long long* out, int* bad) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    Ctx<UB_BM> c;
    c.sm = sm;
    c.N = UB_N;
    c.lane = threadIdx.x;
    c.dt = 0.05;
    c.iL1 = 1.0 / 7.05;
    c.iL2 = 1.0 / 12.45;
    c.Mh = 0.15;
    c.mu = 0.1;
    c.tau = 0.99;
    const int total = UB_SR2 * (UB_N + 1) + kScratch;
    for (int t = c.lane; t < total; t += 64) sm[t] = 1e-3 * (double)((t * 37 + blockIdx.x) % 97);
    __syncthreads();
    if (c.lane < 36) sm[hQW + c.lane] = (c.lane % 7 == 0) ? 1.0 : 0.0;
    if (c.lane < 4) sm[hRW + c.lane] = (c.lane == 0 || c.lane == 3) ? 10.0 : 0.0;
    for (int k = 0; k <= UB_N; ++k)
        for (int q = c.lane; q < 7; q += 64) sm[HEAD + k * SR + (q < 6 ? rHD + q : PAD)] = q < 6 ? 2.0 : 0.0;  // diagonal Hessian rows, zero pad
    __syncthreads();
    bool ok = true;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int r = 0; r < reps; ++r) ok = ub_riccati<V>(c, 1e-4 + 1e-12 * r) && ok;
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (c.lane == 0) out[blockIdx.x] = t1 - t0;
    // checksum of the stage records the sweeps wrote (variants must reproduce phase_riccati bit for bit)
    double cs = 0.0;
    for (int t = c.lane; t < SR * (UB_N + 1); t += 64) cs += sm[HEAD + t] * (double)(1 + (t % 13));
    cs = wsum(cs);
    if (c.lane == 0) out[gridDim.x + blockIdx.x] = (unsigned long long)__double_as_longlong(cs);
    if (!ok && c.lane == 0) atomicAdd(bad, 1);
}

std::vector<unsigned long long> g_ref;  // the shipped phase's checksums (set by its run)

template <int V>
void run(const char* name, int B = 1024) {
    const int reps = 200;
    unsigned long long* d_out;
    int* d_bad;
    (void)hipMalloc(&d_out, 2 * B * sizeof(unsigned long long));
    (void)hipMalloc(&d_bad, sizeof(int));
    (void)hipMemset(d_bad, 0, sizeof(int));
    const int bytes = 8 * (UB_SR2 * (UB_N + 1) + kScratch);
    hipLaunchKernelGGL(ub_kernel<V>, dim3(B), dim3(64), bytes, 0, reps, d_out, d_bad);  // warm-up
    hipLaunchKernelGGL(ub_kernel<V>, dim3(B), dim3(64), bytes, 0, reps, d_out, d_bad);
    (void)hipDeviceSynchronize();
    std::vector<unsigned long long> h(2 * B);
    (void)hipMemcpy(h.data(), d_out, 2 * B * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    double s = 0;
    for (int b = 0; b < B; ++b) s += (double)h[b];
    std::vector<unsigned long long>& ref = g_ref;  // one reference for every instantiation of run<V>
    if (V == 9) ref.assign(h.begin() + B, h.end());
    int diff = 0;
    for (int b = 0; b < B && b < (int)ref.size(); ++b) diff += h[B + b] != ref[b];
    printf("[records vs phase_riccati: %d of %d instances differ] ", diff, B);
    // s_memtime counts at the 100 MHz reference clock on gfx950: report both
    printf("%-44s B=%5d %8.2f memtime ticks/stage\n", name, B, s / B / reps / UB_N);
    (void)hipFree(d_out);
    (void)hipFree(d_bad);
}

__global__ __launch_bounds__(64) void ua_kernel(double* out) {
    __shared__ __attribute__((aligned(16))) double t[256];
    for (int q = threadIdx.x; q < 256; q += 64) t[q] = (double)q + 0.25;
    __syncthreads();
    const int off = 2 * threadIdx.x + 1;  // odd: 8-byte aligned only
    const double2 v = *reinterpret_cast<const double2*>(__builtin_assume_aligned(t + off, 16));
    out[2 * threadIdx.x] = v.x;
    out[2 * threadIdx.x + 1] = v.y;
}

__global__ __launch_bounds__(64) void wred_kernel(const double* in, double* out) {
    const int l = threadIdx.x;
    double a = in[l], b = in[64 + l], c = in[128 + l], d = in[192 + l];
    double e = a, f = b;
    wred4(l, a, b, c, d, OpSum());
    wred2(l, e, f, OpMax());
    double g = in[l], h = in[64 + l], i2 = in[128 + l], j2 = in[192 + l];
    wred4(l, g, h, i2, j2, OpMax());
    if (l == 0) { out[0] = a; out[1] = b; out[2] = c; out[3] = d; out[4] = e; out[5] = f; }
    if (l == 5) { out[6] = g; out[7] = h; out[8] = i2; out[9] = j2; }
}

void check_wred() {
    std::vector<double> h(256);
    for (int t = 0; t < 256; ++t) h[t] = (double)((t * 7919) % 1000) / 7.0 - 50.0;
    double *din, *dout;
    (void)hipMalloc(&din, 256 * sizeof(double));
    (void)hipMalloc(&dout, 16 * sizeof(double));
    (void)hipMemcpy(din, h.data(), 256 * sizeof(double), hipMemcpyHostToDevice);
    hipLaunchKernelGGL(wred_kernel, dim3(1), dim3(64), 0, 0, din, dout);
    double o[16];
    (void)hipMemcpy(o, dout, 10 * sizeof(double), hipMemcpyDeviceToHost);
    double sm[4] = {0, 0, 0, 0}, mx[4] = {-1e300, -1e300, -1e300, -1e300};
    for (int q = 0; q < 4; ++q)
        for (int l = 0; l < 64; ++l) { sm[q] += h[64 * q + l]; mx[q] = std::max(mx[q], h[64 * q + l]); }
    int bad = 0;
    for (int q = 0; q < 4; ++q) bad += std::fabs(o[q] - sm[q]) > 1e-9 * (1 + std::fabs(sm[q]));
    bad += o[4] != mx[0] || o[5] != mx[1];
    for (int q = 0; q < 4; ++q) bad += o[6 + q] != mx[q];
    printf("wred2/wred4: %d wrong (sums %.6f %.6f %.6f %.6f vs %.6f %.6f %.6f %.6f)\n", bad, o[0], o[1], o[2], o[3],
           sm[0], sm[1], sm[2], sm[3]);
    (void)hipFree(din);
    (void)hipFree(dout);
}

void check_unaligned() {
    double* d;
    (void)hipMalloc(&d, 128 * sizeof(double));
    hipLaunchKernelGGL(ua_kernel, dim3(1), dim3(64), 0, 0, d);
    std::vector<double> h(128);
    (void)hipMemcpy(h.data(), d, 128 * sizeof(double), hipMemcpyDeviceToHost);
    int bad = 0;
    for (int l = 0; l < 64; ++l) bad += h[2 * l] != 2 * l + 1.25 || h[2 * l + 1] != 2 * l + 2.25;
    printf("8-byte aligned ds_read_b128: %d of 64 lanes wrong (lane 0: %.2f %.2f)\n", bad, h[0], h[1]);
    (void)hipFree(d);
}

}  // namespace
}  // namespace ttmpc

int main() {
    using namespace ttmpc;
    run<9>("phase_riccati<N=20> (input shift, 4-term)");
    run<60>("round-7 stage (second half unfenced)");
    run<61>("60 + second prefetch half and P^ write fenced");
    run<62>("61 + g_u' by one b128 and selects");
    run<63>("61 + factor-row store one stage later");
    run<64>("61 + both");
    run<65>("60 + factor-row store one stage later");
    run<66>("60 + PA first, H_uu inverse behind the tile reads (= shipped)");
    run<67>("60 + PA first + late store");
    run<68>("61 + PA first + late store");
    run<69>("66 + g_u' by one b128 and selects");
    run<70>("66, first prefetch half unfenced");
    run<71>("66, both prefetch halves behind the PA reads");
    run<50>("round-5 stage (6-term)");
    run<51>("round-5 stage, no prefetch, no store");
    run<9>("phase_riccati<N=20> (again)");
    run<60>("round-7 stage (again)");
    run<9>("phase_riccati<N=20> B=256", 256);
    run<60>("round-7 stage B=256", 256);
    run<61>("60 + fenced B=256", 256);
    run<62>("61 + g_u' by one b128 and selects B=256", 256);
    run<63>("61 + factor-row store one stage later B=256", 256);
    run<64>("61 + both B=256", 256);
    run<65>("60 + late store B=256", 256);
    run<66>("60 + PA first (= shipped) B=256", 256);
    run<67>("60 + PA first + late store B=256", 256);
    run<68>("61 + PA first + late store B=256", 256);
    run<69>("66 + g select B=256", 256);
    run<70>("66, first half unfenced B=256", 256);
    run<71>("66, both halves behind the PA reads B=256", 256);
    run<50>("round-5 stage B=256", 256);
    check_unaligned();
    check_wred();
    return 0;
}
