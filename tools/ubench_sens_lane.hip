// Micro-benchmark: the one-instance-per-lane candidate for the x_init sensitivity pass (DESIGN.md "Multiplier export and
// x_init sensitivities").  The shipped track_sens_kernel (csrc/tt_sens.hip) gives one wavefront to an instance; this is
// the other obvious mapping: a lane runs the whole recursion of its instance in registers (P 36, Phi 36 doubles), the
// gains K_k go through a global workspace laid out [k][12][B] so that the lanes' accesses coalesce.  Same work per
// instance as the shipped kernel (3 sincos and the 9 + 7 model entries per stage, the sparse A products, a 2x2 solve, the
// forward sweep), on synthetic inputs: it is a timing candidate, checked only for finite, non-trivial output.
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/ubench_sens_lane.hip -o tools/bin/ubench_sens_lane
//   tools/bin/ubench_sens_lane [B=1024] [N=20]
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

struct Par { int N, B; double dt, iL1, iL2, Mh; };

__device__ __forceinline__ void stage_model(const Par& p, const double* x, const double* y, double* aj, double* wc) {
    double sth, cth, sps, cps, sph, cph;
    sincos(x[2], &sth, &cth);
    sincos(x[3], &sps, &cps);
    sincos(x[4], &sph, &cph);
    const double v = x[5], dt = p.dt, iL1 = p.iL1, iL2 = p.iL2, Mh = p.Mh, iL1L2 = iL1 * iL2;
    const double ic = 1.0 / cph, t = sph * ic, c2 = ic * ic, kk = 1.0 + Mh * iL2 * cps;
    aj[0] = dt * (-v * sth); aj[1] = dt * cth; aj[2] = dt * (v * cth); aj[3] = dt * sth;
    aj[4] = dt * (v * c2 * iL1); aj[5] = dt * (t * iL1);
    aj[6] = dt * (v * t * Mh * sps * iL1L2 - v * cps * iL2);
    aj[7] = dt * (-v * c2 * iL1 * kk);
    aj[8] = dt * (-t * iL1 * kk - sps * iL2);
    const double s = -dt;
    wc[0] = s * (y[0] * (-v * cth) + y[1] * (-v * sth));
    wc[1] = s * (y[0] * (-sth) + y[1] * cth);
    wc[2] = s * (y[3] * (v * t * Mh * cps * iL1L2 + v * sps * iL2));
    wc[3] = s * (y[3] * (v * c2 * Mh * sps * iL1L2));
    wc[4] = s * (y[3] * (t * Mh * sps * iL1L2 - cps * iL2));
    wc[5] = s * (y[2] * (2.0 * v * t * c2 * iL1) + y[3] * (-2.0 * v * t * c2 * kk * iL1));
    wc[6] = s * (y[2] * (c2 * iL1) + y[3] * (-c2 * kk * iL1));
}

// x [B][N+1][6], dual [B][N+1][22] (y | z_L | z_U), ws [N][12][B]; outputs gain [B][12], and with FULL dxdx0, dudx0
template <bool FULL>
__global__ __launch_bounds__(64) void sens_lane(Par p, const double* x, const double* dual, double* ws, double* gain,
                                                double* dxdx0, double* dudx0) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const int N = p.N, S = N + 1;
    const double dt = p.dt;
    const double* xb = x + (size_t)b * S * 6;
    const double* db = dual + (size_t)b * S * 22;
    double P[6][6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) P[i][j] = i == j ? 2.0 + db[N * 22 + 6 + i] + db[N * 22 + 14 + i] : 0.0;
    for (int k = N - 1; k >= 0; --k) {
        double xs[6], y1[6], aj[9], wc[7], sg[8];
#pragma unroll
        for (int i = 0; i < 6; ++i) { xs[i] = xb[k * 6 + i]; y1[i] = db[(k + 1) * 22 + i]; }
#pragma unroll
        for (int v = 0; v < 8; ++v) sg[v] = db[k * 22 + 6 + v] / 0.5 + db[k * 22 + 14 + v] / 0.5;  // two divisions per variable
        stage_model(p, xs, y1, aj, wc);
        double M[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            M[i][0] = P[i][0];
            M[i][1] = P[i][1];
            M[i][2] = P[i][2] + aj[0] * P[i][0] + aj[2] * P[i][1];
            M[i][3] = P[i][3] + aj[6] * P[i][3];
            M[i][4] = P[i][4] + aj[4] * P[i][2] + aj[7] * P[i][3];
            M[i][5] = P[i][5] + aj[1] * P[i][0] + aj[3] * P[i][1] + aj[5] * P[i][2] + aj[8] * P[i][3];
        }
        const double g00 = 20.0 + sg[6] + dt * dt * P[5][5], g01 = dt * dt * P[5][4], g11 = 20.0 + sg[7] + dt * dt * P[4][4];
        const double idet = 1.0 / (g00 * g11 - g01 * g01);
        double K[2][6];
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double h0 = dt * M[5][j], h1 = dt * M[4][j];
            K[0][j] = (g11 * h0 - g01 * h1) * idet;
            K[1][j] = (g00 * h1 - g01 * h0) * idet;
            ws[((size_t)k * 12 + j) * p.B + b] = K[0][j];
            ws[((size_t)k * 12 + 6 + j) * p.B + b] = K[1][j];
        }
        if (k > 0) {
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double c[6];
                c[0] = M[0][j];
                c[1] = M[1][j];
                c[2] = M[2][j] + aj[0] * M[0][j] + aj[2] * M[1][j];
                c[3] = M[3][j] + aj[6] * M[3][j];
                c[4] = M[4][j] + aj[4] * M[2][j] + aj[7] * M[3][j];
                c[5] = M[5][j] + aj[1] * M[0][j] + aj[3] * M[1][j] + aj[5] * M[2][j] + aj[8] * M[3][j];
#pragma unroll
                for (int i = 0; i < 6; ++i)
                    P[i][j] = (i == j ? 2.0 + sg[i] : 0.0) + c[i] - (dt * M[5][i] * K[0][j] + dt * M[4][i] * K[1][j]);
            }
            P[2][2] += wc[0]; P[2][5] += wc[1]; P[5][2] += wc[1]; P[3][3] += wc[2]; P[3][4] += wc[3]; P[4][3] += wc[3];
            P[3][5] += wc[4]; P[5][3] += wc[4]; P[4][4] += wc[5]; P[4][5] += wc[6]; P[5][4] += wc[6];
        } else {
#pragma unroll
            for (int j = 0; j < 6; ++j) { gain[(size_t)b * 12 + j] = -K[0][j]; gain[(size_t)b * 12 + 6 + j] = -K[1][j]; }
        }
    }
    if constexpr (FULL) {
        double F[6][6];
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = 0; j < 6; ++j) { F[i][j] = i == j ? 1.0 : 0.0; dxdx0[(size_t)b * S * 36 + i * 6 + j] = F[i][j]; }
        for (int k = 0; k < N; ++k) {
            double xs[6], y1[6] = {0, 0, 0, 0, 0, 0}, aj[9], wc[7], K[2][6];
#pragma unroll
            for (int i = 0; i < 6; ++i) xs[i] = xb[k * 6 + i];
            stage_model(p, xs, y1, aj, wc);  // A_k again (recomputed rather than stored)
#pragma unroll
            for (int j = 0; j < 6; ++j) { K[0][j] = ws[((size_t)k * 12 + j) * p.B + b]; K[1][j] = ws[((size_t)k * 12 + 6 + j) * p.B + b]; }
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                double d0 = 0.0, d1 = 0.0;
#pragma unroll
                for (int l = 0; l < 6; ++l) { d0 -= K[0][l] * F[l][j]; d1 -= K[1][l] * F[l][j]; }
                dudx0[((size_t)b * N + k) * 12 + j] = d0;
                dudx0[((size_t)b * N + k) * 12 + 6 + j] = d1;
                double c[6];
                c[0] = F[0][j] + aj[0] * F[2][j] + aj[1] * F[5][j];
                c[1] = F[1][j] + aj[2] * F[2][j] + aj[3] * F[5][j];
                c[2] = F[2][j] + aj[4] * F[4][j] + aj[5] * F[5][j];
                c[3] = F[3][j] + aj[6] * F[3][j] + aj[7] * F[4][j] + aj[8] * F[5][j];
                c[4] = F[4][j] + dt * d1;
                c[5] = F[5][j] + dt * d0;
#pragma unroll
                for (int i = 0; i < 6; ++i) { F[i][j] = c[i]; dxdx0[((size_t)b * S + k + 1) * 36 + i * 6 + j] = c[i]; }
            }
        }
    }
}

int main(int argc, char** argv) {
    const int B = argc > 1 ? atoi(argv[1]) : 1024, N = argc > 2 ? atoi(argv[2]) : 20, S = N + 1;
    if (B < 1 || N < 1 || N > 200) return 2;
    Par p = {N, B, 0.05, 1.0 / 7.05, 1.0 / 12.45, 0.15};
    std::vector<double> hx((size_t)B * S * 6), hd((size_t)B * S * 22);
    for (int b = 0; b < B; ++b)
        for (int k = 0; k < S; ++k) {
            double* x = &hx[((size_t)b * S + k) * 6];
            x[0] = 0.1 * k; x[1] = 0.05 * k + b % 7; x[2] = 0.3 * sin(0.1 * k + b); x[3] = 0.2 * cos(0.07 * k + b);
            x[4] = 0.1 * sin(0.05 * k + 2 * b); x[5] = 2.0 + 0.01 * k;
            double* d = &hd[((size_t)b * S + k) * 22];
            for (int i = 0; i < 6; ++i) d[i] = 0.1 * sin(i + k + b);
            for (int i = 6; i < 22; ++i) d[i] = 1e-9;
        }
    double *dx, *dd, *ws, *gain, *dX, *dU;
    CK(hipMalloc(&dx, hx.size() * 8)); CK(hipMalloc(&dd, hd.size() * 8)); CK(hipMalloc(&ws, (size_t)N * 12 * B * 8));
    CK(hipMalloc(&gain, (size_t)B * 12 * 8)); CK(hipMalloc(&dX, (size_t)B * S * 36 * 8)); CK(hipMalloc(&dU, (size_t)B * N * 12 * 8));
    CK(hipMemcpy(dx, hx.data(), hx.size() * 8, hipMemcpyHostToDevice));
    CK(hipMemcpy(dd, hd.data(), hd.size() * 8, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const int blocks = (B + 63) / 64, reps = 200;
    for (int full = 0; full < 2; ++full) {
        for (int rnd = 0; rnd < 3; ++rnd) {
            for (int i = 0; i < 10 + reps; ++i) {
                if (i == 10) CK(hipEventRecord(e0, 0));
                if (full) hipLaunchKernelGGL(sens_lane<true>, dim3(blocks), dim3(64), 0, 0, p, dx, dd, ws, gain, dX, dU);
                else hipLaunchKernelGGL(sens_lane<false>, dim3(blocks), dim3(64), 0, 0, p, dx, dd, ws, gain, dX, dU);
            }
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            CK(hipGetLastError());
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            printf("lane-per-instance B=%d N=%d %s: %.2f us/launch\n", B, N, full ? "gain+trajectory" : "gain only", 1e3 * ms / reps);
        }
    }
    std::vector<double> hg((size_t)B * 12);
    CK(hipMemcpy(hg.data(), gain, hg.size() * 8, hipMemcpyDeviceToHost));
    double mx = 0; bool fin = true;
    for (double v : hg) { fin = fin && isfinite(v); mx = fmax(mx, fabs(v)); }
    printf("gain finite %d, max|K| %.4f\n", (int)fin, mx);
    return fin && mx > 0 ? 0 : 1;
}
