// SE(3) pose-graph optimisation in fp64: the g2o subset the reference's back end runs
// (slam/pose_graph_optimization.py: g2o.SparseOptimizer + BlockSolverSE3 + OptimizationAlgorithmLevenberg over VertexSE3 /
// EdgeSE3; slam/slam.py:110-115,203-246 builds it and calls optimize(max_iterations=10000) at every loop closure).
// The Levenberg control runs on the host (clslam_hip/pose_graph.py); these kernels are its linear algebra.
//
// Conventions (g2o types/slam3d, restated from its published source; not checked against a g2o build):
//   pose       X = [R t; 0 1], stored as a row-major 4x4 of doubles.
//   chart      v = (t, qxyz) -> exp(v) = [R(q) t], q = (w = sqrt(1 - |qxyz|^2), qxyz); |qxyz|^2 > 1 gives R = I
//              (fromVectorMQT / fromCompactQuaternion).
//   update     VertexSE3 moves by RIGHT multiplication X <- X * exp(v); fixed vertices never move.  g2o re-orthonormalises
//              R every 1000 updates (approximateNearestOrthogonalMatrix: R -= 0.5 R (R^T R - I)); here every update does it.
//   error      e = toVectorMQT(Z^-1 * Xi^-1 * Xj), i = vertex(0), j = vertex(1): translation, then the xyz part of the unit
//              quaternion of the rotation (Eigen's matrix->quaternion conversion), its sign chosen so that w >= 0.
//   chi2       e^T Omega e with Omega used symmetrised, (Omega + Omega^T) / 2 (the host symmetrises it on entry; g2o differs
//              only for an asymmetric Omega).
//   Huber      s = chi2: rho = s for s <= d^2, else 2 d sqrt(s) - d^2; H and b are weighted by rho'(s), the LM scores sum(rho).
//   Jacobians  A = de/dv_i, B = de/dv_j at v = 0 by central differences in fp64 (step kJacStep).
//   system     H = sum J^T W J, b = sum J^T W e (W = rho' Omega) over the ACTIVE vertices: not fixed and in at least one
//              edge (g2o's initializeOptimization leaves isolated vertices out).  The step solves (H + lambda I) d = -b.
//
// Kernels (no floating-point atomics anywhere: the whole optimisation is bitwise reproducible from run to run):
//   pgo_linearize_kernel   one work item per edge: e, A, B -> A^T W A, A^T W B, B^T W B, A^T W e, B^T W e, rho
//   pgo_assemble_kernel    one work item per 6x6 block of the block-CSR H (and per row of b): the per-edge blocks summed
//                          over a contribution list built on the host, in its fixed order
//   pgo_solve_kernel       ONE workgroup: preconditioned conjugate gradients, vectors in global memory (L2-resident),
//                          __syncthreads() between phases, no host round trip per CG iteration.  Preconditioner: the block-
//                          tridiagonal part of H + lambda I over consecutive active indices (the host orders active vertices
//                          by id, so it is exact on slam.py's odometry chain), factored once per solve by block cyclic
//                          reduction and applied in 2 log2(n) dependent steps.  It is SPD for any pose graph: every edge
//                          term it keeps is a PSD block of J^T W J.  Stop: ||r|| <= tol ||b|| or the iteration cap.
//   pgo_update_score_kernel ONE workgroup: trial = X * exp(d) for the active vertices (a copy), then sum(rho) over the edges
//                          with a fixed-order tree reduction.
#include "common.h"

#include <cmath>

namespace clslam {

constexpr double kJacStep = 1e-6;   // central-difference step: truncation ~1e-12, rounding ~1e-10
#if CLSLAM_DEVICE_BUILD
constexpr int kPgoThreads = 512;   // single-workgroup kernels: 8 waves, 2 per SIMD (256 VGPRs of room for the 6x6 fp64 blocks)
#else
constexpr int kPgoThreads = 256;
#endif
constexpr int kLinStride = 128;     // per-edge record of pgo_linearize_kernel (doubles)
enum { kLinHii = 0, kLinHij = 36, kLinHjj = 72, kLinBi = 108, kLinBj = 114, kLinRho = 120 };

struct Iso {
    double R[9];   // row-major
    double t[3];
};

__device__ __forceinline__ void iso_load(const double* m, Iso& X) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) X.R[r * 3 + c] = m[r * 4 + c];
        X.t[r] = m[r * 4 + 3];
    }
}

__device__ __forceinline__ void iso_store(const Iso& X, double* m) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m[r * 4 + c] = X.R[r * 3 + c];
        m[r * 4 + 3] = X.t[r];
    }
    m[12] = 0.0; m[13] = 0.0; m[14] = 0.0; m[15] = 1.0;
}

__device__ __forceinline__ void iso_mul(const Iso& a, const Iso& b, Iso& c) {
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k)
            c.R[r * 3 + k] = a.R[r * 3 + 0] * b.R[0 * 3 + k] + a.R[r * 3 + 1] * b.R[1 * 3 + k] + a.R[r * 3 + 2] * b.R[2 * 3 + k];
        c.t[r] = a.R[r * 3 + 0] * b.t[0] + a.R[r * 3 + 1] * b.t[1] + a.R[r * 3 + 2] * b.t[2] + a.t[r];
    }
}

__device__ __forceinline__ void iso_inv(const Iso& a, Iso& c) {
    for (int r = 0; r < 3; ++r)
        for (int k = 0; k < 3; ++k) c.R[r * 3 + k] = a.R[k * 3 + r];
    for (int r = 0; r < 3; ++r) c.t[r] = -(c.R[r * 3 + 0] * a.t[0] + c.R[r * 3 + 1] * a.t[1] + c.R[r * 3 + 2] * a.t[2]);
}

// fromVectorMQT
__device__ __forceinline__ void iso_exp(const double* v, Iso& X) {
    const double x = v[3], y = v[4], z = v[5];
    const double w2 = 1.0 - (x * x + y * y + z * z);
    if (w2 < 0.0) {
        for (int i = 0; i < 9; ++i) X.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    } else {
        const double w = sqrt(w2);
        X.R[0] = 1.0 - 2.0 * (y * y + z * z); X.R[1] = 2.0 * (x * y - z * w);       X.R[2] = 2.0 * (x * z + y * w);
        X.R[3] = 2.0 * (x * y + z * w);       X.R[4] = 1.0 - 2.0 * (x * x + z * z); X.R[5] = 2.0 * (y * z - x * w);
        X.R[6] = 2.0 * (x * z - y * w);       X.R[7] = 2.0 * (y * z + x * w);       X.R[8] = 1.0 - 2.0 * (x * x + y * y);
    }
    X.t[0] = v[0]; X.t[1] = v[1]; X.t[2] = v[2];
}

// toVectorMQT: Eigen's rotation-matrix -> quaternion, normalised, w >= 0
__device__ __forceinline__ void iso_log(const Iso& X, double* e) {
    const double* m = X.R;
    double q[4];   // x y z w
    double t = m[0] + m[4] + m[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(m[i * 4] - m[j * 4] - m[k * 4] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t;
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t;
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t;
    }
    double n = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (q[3] < 0.0) n = -n;
    e[0] = X.t[0]; e[1] = X.t[1]; e[2] = X.t[2];
    e[3] = q[0] * n; e[4] = q[1] * n; e[5] = q[2] * n;
}

// X <- X * exp(v), then one step of approximateNearestOrthogonalMatrix
__device__ __forceinline__ void iso_oplus(const Iso& X, const double* v, Iso& out) {
    Iso d;
    iso_exp(v, d);
    iso_mul(X, d, out);
    double E[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            E[r * 3 + c] = out.R[0 * 3 + r] * out.R[0 * 3 + c] + out.R[1 * 3 + r] * out.R[1 * 3 + c] +
                           out.R[2 * 3 + r] * out.R[2 * 3 + c] - (r == c ? 1.0 : 0.0);
    double Rn[9];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c)
            Rn[r * 3 + c] = out.R[r * 3 + c] - 0.5 * (out.R[r * 3 + 0] * E[0 * 3 + c] + out.R[r * 3 + 1] * E[1 * 3 + c] +
                                                      out.R[r * 3 + 2] * E[2 * 3 + c]);
    for (int i = 0; i < 9; ++i) out.R[i] = Rn[i];
}

// e = toVectorMQT(Zinv * Xi^-1 * Xj)
__device__ __forceinline__ void edge_error(const Iso& Zinv, const Iso& Xi, const Iso& Xj, double* e) {
    Iso a, b, c;
    iso_inv(Xi, a);
    iso_mul(a, Xj, b);
    iso_mul(Zinv, b, c);
    iso_log(c, e);
}

// e, A = de/dv_i, B = de/dv_j (column-major in k: A[r*6+k] = de_r/dv_k)
__device__ void edge_eval(const double* Xi_m, const double* Xj_m, const double* Z_m, double* e, double* A, double* B) {
    Iso Xi, Xj, Z, Zinv, P;
    iso_load(Xi_m, Xi); iso_load(Xj_m, Xj); iso_load(Z_m, Z);
    iso_inv(Z, Zinv);
    edge_error(Zinv, Xi, Xj, e);
    for (int side = 0; side < 2; ++side) {
        double* J = side ? B : A;
        for (int k = 0; k < 6; ++k) {
            double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, ep[6], em[6];
            v[k] = kJacStep;
            Iso d;
            iso_exp(v, d);
            iso_mul(side ? Xj : Xi, d, P);
            if (side) edge_error(Zinv, Xi, P, ep); else edge_error(Zinv, P, Xj, ep);
            v[k] = -kJacStep;
            iso_exp(v, d);
            iso_mul(side ? Xj : Xi, d, P);
            if (side) edge_error(Zinv, Xi, P, em); else edge_error(Zinv, P, Xj, em);
            for (int r = 0; r < 6; ++r) J[r * 6 + k] = (ep[r] - em[r]) / (2.0 * kJacStep);
        }
    }
}

__device__ __forceinline__ double quad_form(const double* W, const double* e) {
    double s = 0.0;
    for (int r = 0; r < 6; ++r) {
        double we = 0.0;
        for (int c = 0; c < 6; ++c) we += W[r * 6 + c] * e[c];
        s += e[r] * we;
    }
    return s;
}

// (rho(s), rho'(s)) of RobustKernelHuber(delta); delta <= 0: no robust kernel
__device__ __forceinline__ void huber(double s, double delta, double* rho, double* drho) {
    if (delta <= 0.0 || s <= delta * delta) { *rho = s; *drho = 1.0; return; }
    const double r = sqrt(s);
    *rho = 2.0 * delta * r - delta * delta;
    *drho = delta / r;
}

__global__ __launch_bounds__(64) void pgo_edge_eval_kernel(const double* __restrict__ est, const int* __restrict__ ev,
                                                           const double* __restrict__ meas, int ne, double* __restrict__ err,
                                                           double* __restrict__ jac_i, double* __restrict__ jac_j) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= ne) return;
    edge_eval(est + (size_t)ev[2 * k] * 16, est + (size_t)ev[2 * k + 1] * 16, meas + (size_t)k * 16, err + (size_t)k * 6,
              jac_i + (size_t)k * 36, jac_j + (size_t)k * 36);
}

__global__ __launch_bounds__(64) void pgo_linearize_kernel(const double* __restrict__ est, const int* __restrict__ ev,
                                                           const double* __restrict__ meas, const double* __restrict__ info,
                                                           const double* __restrict__ delta, int ne, double* __restrict__ lin) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= ne) return;
    double e[6], A[36], B[36];
    edge_eval(est + (size_t)ev[2 * k] * 16, est + (size_t)ev[2 * k + 1] * 16, meas + (size_t)k * 16, e, A, B);
    const double* Om = info + (size_t)k * 36;
    double rho, w;
    huber(quad_form(Om, e), delta[k], &rho, &w);
    double* out = lin + (size_t)k * kLinStride;
    double WA[36], WB[36], We[6];   // W = w * Omega
    for (int r = 0; r < 6; ++r) {
        double se = 0.0;
        for (int c = 0; c < 6; ++c) {
            double sa = 0.0, sb = 0.0;
            for (int m = 0; m < 6; ++m) { sa += Om[r * 6 + m] * A[m * 6 + c]; sb += Om[r * 6 + m] * B[m * 6 + c]; }
            WA[r * 6 + c] = w * sa; WB[r * 6 + c] = w * sb;
            se += Om[r * 6 + c] * e[c];
        }
        We[r] = w * se;
    }
    for (int r = 0; r < 6; ++r) {
        for (int c = 0; c < 6; ++c) {
            double hii = 0.0, hij = 0.0, hjj = 0.0;
            for (int m = 0; m < 6; ++m) {
                hii += A[m * 6 + r] * WA[m * 6 + c];
                hij += A[m * 6 + r] * WB[m * 6 + c];
                hjj += B[m * 6 + r] * WB[m * 6 + c];
            }
            out[kLinHii + r * 6 + c] = hii; out[kLinHij + r * 6 + c] = hij; out[kLinHjj + r * 6 + c] = hjj;
        }
        double bi = 0.0, bj = 0.0;
        for (int m = 0; m < 6; ++m) { bi += A[m * 6 + r] * We[m]; bj += B[m * 6 + r] * We[m]; }
        out[kLinBi + r] = bi; out[kLinBj + r] = bj;
    }
    out[kLinRho] = rho;
}

// Work item q < nnzb: block q of H = sum of its contributions contrib[cptr[q] .. cptr[q+1]) (code = edge*4 + kind;
// kind 0 Hii, 1 Hjj, 2 Hij, 3 Hij^T).  Work item nnzb + r: b of active row r from the contributions of its diagonal block
// diag[r] (kinds 0 / 1 carry bi / bj).
__global__ __launch_bounds__(256) void pgo_assemble_kernel(const double* __restrict__ lin, const int* __restrict__ cptr,
                                                           const int* __restrict__ contrib, const int* __restrict__ diag, int nnzb,
                                                           int na, double* __restrict__ H, double* __restrict__ b) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w < nnzb) {
        double s[36];
        for (int i = 0; i < 36; ++i) s[i] = 0.0;
        for (int c = cptr[w]; c < cptr[w + 1]; ++c) {
            const int code = contrib[c], kind = code & 3;
            const double* L = lin + (size_t)(code >> 2) * kLinStride;
            if (kind == 3) {
                for (int r = 0; r < 6; ++r)
                    for (int cc = 0; cc < 6; ++cc) s[r * 6 + cc] += L[kLinHij + cc * 6 + r];
            } else {
                const double* src = L + (kind == 0 ? kLinHii : kind == 1 ? kLinHjj : kLinHij);
                for (int i = 0; i < 36; ++i) s[i] += src[i];
            }
        }
        for (int i = 0; i < 36; ++i) H[(size_t)w * 36 + i] = s[i];
    } else if (w < nnzb + na) {
        const int r = w - nnzb, q = diag[r];
        double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int c = cptr[q]; c < cptr[q + 1]; ++c) {
            const int code = contrib[c], kind = code & 3;
            if (kind > 1) continue;
            const double* L = lin + (size_t)(code >> 2) * kLinStride + (kind == 0 ? kLinBi : kLinBj);
            for (int i = 0; i < 6; ++i) s[i] += L[i];
        }
        for (int i = 0; i < 6; ++i) b[(size_t)r * 6 + i] = s[i];
    }
}

// ---- single-workgroup helpers ---------------------------------------------------------------------------------------
// fixed-order block reduction: thread partials, then a tree over kPgoThreads slots; every thread gets the total
__device__ double block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int st = kPgoThreads / 2; st >= 1; st >>= 1) {
        if (tid < st) red[tid] += red[tid + st];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

__device__ double block_max(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int st = kPgoThreads / 2; st >= 1; st >>= 1) {
        if (tid < st) red[tid] = red[tid] > red[tid + st] ? red[tid] : red[tid + st];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

__device__ double dot(const double* a, const double* b, int n, double* red) {
    double s = 0.0;
    for (int w = threadIdx.x; w < n; w += kPgoThreads) s += a[w] * b[w];
    return block_sum(s, red);
}

// C = A * B (6x6), optionally negated
__device__ __forceinline__ void mm6(const double* A, const double* B, double* C, double sign) {
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) {
            double s = 0.0;
            for (int m = 0; m < 6; ++m) s += A[r * 6 + m] * B[m * 6 + c];
            C[r * 6 + c] = sign * s;
        }
}

// y (+)= sign * A x (6x6)
__device__ __forceinline__ void mv6_acc(const double* A, const double* x, double* y, double sign) {
    for (int r = 0; r < 6; ++r) {
        double s = 0.0;
        for (int m = 0; m < 6; ++m) s += A[r * 6 + m] * x[m];
        y[r] += sign * s;
    }
}

// inverse of a 6x6 (SPD in use) by Gauss-Jordan with partial pivoting; false when singular
__device__ bool inv6(const double* M, double* Inv) {
    double a[36];
    for (int i = 0; i < 36; ++i) { a[i] = M[i]; Inv[i] = (i % 7 == 0) ? 1.0 : 0.0; }
    for (int c = 0; c < 6; ++c) {
        int p = c;
        for (int r = c + 1; r < 6; ++r)
            if (fabs(a[r * 6 + c]) > fabs(a[p * 6 + c])) p = r;
        if (!(fabs(a[p * 6 + c]) > 0.0)) return false;
        if (p != c)
            for (int k = 0; k < 6; ++k) {
                double t = a[c * 6 + k]; a[c * 6 + k] = a[p * 6 + k]; a[p * 6 + k] = t;
                t = Inv[c * 6 + k]; Inv[c * 6 + k] = Inv[p * 6 + k]; Inv[p * 6 + k] = t;
            }
        const double d = 1.0 / a[c * 6 + c];
        for (int k = 0; k < 6; ++k) { a[c * 6 + k] *= d; Inv[c * 6 + k] *= d; }
        for (int r = 0; r < 6; ++r) {
            if (r == c) continue;
            const double f = a[r * 6 + c];
            if (f == 0.0) continue;
            for (int k = 0; k < 6; ++k) { a[r * 6 + k] -= f * a[c * 6 + k]; Inv[r * 6 + k] -= f * Inv[c * 6 + k]; }
        }
    }
    return true;
}

struct CrWork {
    double *A, *B, *C, *Binv, *AG;   // [na][36] x4, AG: [sum over levels of kept rows][72] (alpha | gamma)
};

// Block cyclic reduction of the block-tridiagonal M: row k couples to k-1 (A_k), k (B_k), k+1 (C_k).  Level s = 1, 2, 4, ...
// eliminates the rows k = s (mod 2s) from the equations of the kept rows i = 0 (mod 2s):
//   alpha = -A_i B_{i-s}^-1, gamma = -C_i B_{i+s}^-1, B_i += alpha C_{i-s} + gamma A_{i+s}, A_i = alpha A_{i-s}, C_i = gamma C_{i+s}.
// Returns false (every thread) when a pivot block is singular.
__device__ bool cr_factor(const double* __restrict__ H, const int* __restrict__ tri, double lambda, int na, CrWork w,
                          double* red) {
    const int tid = threadIdx.x;
    for (int k = tid; k < na; k += kPgoThreads) {
        const int q0 = tri[3 * k], q1 = tri[3 * k + 1], q2 = tri[3 * k + 2];
        for (int i = 0; i < 36; ++i) {
            w.A[(size_t)k * 36 + i] = q0 >= 0 ? H[(size_t)q0 * 36 + i] : 0.0;
            w.B[(size_t)k * 36 + i] = H[(size_t)q1 * 36 + i] + (i % 7 == 0 ? lambda : 0.0);
            w.C[(size_t)k * 36 + i] = q2 >= 0 ? H[(size_t)q2 * 36 + i] : 0.0;
        }
    }
    __syncthreads();
    double bad = 0.0;
    int off = 0;
    for (int s = 1; s < na; s <<= 1) {
        for (int k = s + 2 * s * tid; k < na; k += 2 * s * kPgoThreads)
            if (!inv6(w.B + (size_t)k * 36, w.Binv + (size_t)k * 36)) bad = 1.0;
        __syncthreads();
        const int cnt = (na - 1) / (2 * s) + 1;
        for (int m = tid; m < cnt; m += kPgoThreads) {
            const int i = m * 2 * s;
            double* al = w.AG + (size_t)(off + m) * 72;
            double* ga = al + 36;
            double T[36];
            if (i >= s) {
                mm6(w.A + (size_t)i * 36, w.Binv + (size_t)(i - s) * 36, al, -1.0);
                mm6(al, w.C + (size_t)(i - s) * 36, T, 1.0);
                for (int x = 0; x < 36; ++x) w.B[(size_t)i * 36 + x] += T[x];
                mm6(al, w.A + (size_t)(i - s) * 36, T, 1.0);
                for (int x = 0; x < 36; ++x) w.A[(size_t)i * 36 + x] = T[x];
            } else {
                for (int x = 0; x < 36; ++x) al[x] = 0.0;
            }
            if (i + s < na) {
                mm6(w.C + (size_t)i * 36, w.Binv + (size_t)(i + s) * 36, ga, -1.0);
                mm6(ga, w.A + (size_t)(i + s) * 36, T, 1.0);
                for (int x = 0; x < 36; ++x) w.B[(size_t)i * 36 + x] += T[x];
                mm6(ga, w.C + (size_t)(i + s) * 36, T, 1.0);
                for (int x = 0; x < 36; ++x) w.C[(size_t)i * 36 + x] = T[x];
            } else {
                for (int x = 0; x < 36; ++x) ga[x] = 0.0;
            }
        }
        __syncthreads();
        off += cnt;
    }
    if (tid == 0 && !inv6(w.B, w.Binv)) bad = 1.0;
    __syncthreads();
    return block_max(bad, red) == 0.0;
}

// z = M^-1 r (z may not alias r)
__device__ void cr_apply(const double* __restrict__ r, double* __restrict__ z, int na, CrWork w) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 6 * na; i += kPgoThreads) z[i] = r[i];
    __syncthreads();
    int off = 0, stop = 0;
    for (int s = 1; s < na; s <<= 1) {                         // forward: f_i += alpha f_{i-s} + gamma f_{i+s}
        const int cnt = (na - 1) / (2 * s) + 1;
        for (int m = tid; m < cnt; m += kPgoThreads) {
            const int i = m * 2 * s;
            const double* al = w.AG + (size_t)(off + m) * 72;
            double f[6];
            for (int x = 0; x < 6; ++x) f[x] = z[(size_t)i * 6 + x];
            if (i >= s) mv6_acc(al, z + (size_t)(i - s) * 6, f, 1.0);
            if (i + s < na) mv6_acc(al + 36, z + (size_t)(i + s) * 6, f, 1.0);
            for (int x = 0; x < 6; ++x) z[(size_t)i * 6 + x] = f[x];
        }
        __syncthreads();
        off += cnt;
        stop = s;
    }
    if (tid == 0) {
        double f[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        mv6_acc(w.Binv, z, f, 1.0);
        for (int x = 0; x < 6; ++x) z[x] = f[x];
    }
    __syncthreads();
    for (int s = stop; s >= 1; s >>= 1) {                       // back substitution of the rows eliminated at level s
        for (int k = s + 2 * s * tid; k < na; k += 2 * s * kPgoThreads) {
            double t[6], x6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            for (int x = 0; x < 6; ++x) t[x] = z[(size_t)k * 6 + x];
            mv6_acc(w.A + (size_t)k * 36, z + (size_t)(k - s) * 6, t, -1.0);
            if (k + s < na) mv6_acc(w.C + (size_t)k * 36, z + (size_t)(k + s) * 6, t, -1.0);
            mv6_acc(w.Binv + (size_t)k * 36, t, x6, 1.0);
            for (int x = 0; x < 6; ++x) z[(size_t)k * 6 + x] = x6[x];
        }
        __syncthreads();
    }
}

// y = (H + lambda I) x over the block-CSR H
__device__ void spmv(const double* __restrict__ H, const int* __restrict__ rptr, const int* __restrict__ col, double lambda,
                     const double* __restrict__ x, double* __restrict__ y, int na) {
    for (int w = threadIdx.x; w < 6 * na; w += kPgoThreads) {
        const int row = w / 6, c = w - row * 6;
        double s = lambda * x[w];
        for (int q = rptr[row]; q < rptr[row + 1]; ++q) {
            const double* Hb = H + (size_t)q * 36 + c * 6;
            const double* xb = x + (size_t)col[q] * 6;
            for (int k = 0; k < 6; ++k) s += Hb[k] * xb[k];
        }
        y[w] = s;
    }
    __syncthreads();
}

// scal out: [1] CG iterations, [2] final relative residual, [3] d^T (lambda d - b) (the model decrease g2o's Levenberg divides
// by: its b is -J^T W e), [5] 1 when the preconditioner could not be factored (d = 0 then).  work: 5 * 6 na doubles.
__global__ __launch_bounds__(kPgoThreads) void pgo_solve_kernel(const double* __restrict__ H, const int* __restrict__ rptr,
                                                                const int* __restrict__ col, const int* __restrict__ tri,
                                                                const double* __restrict__ b, double lambda, int na, double tol,
                                                                int max_iter, double* __restrict__ d, double* __restrict__ vec,
                                                                CrWork cw, double* __restrict__ scal) {
    __shared__ double red[kPgoThreads];
    const int n = 6 * na, tid = threadIdx.x;
    double* r = vec;
    double* z = vec + n;
    double* p = vec + 2 * (size_t)n;
    double* q = vec + 3 * (size_t)n;
    for (int w = tid; w < n; w += kPgoThreads) { d[w] = 0.0; r[w] = -b[w]; }
    __syncthreads();
    const bool ok = cr_factor(H, tri, lambda, na, cw, red);
    const double rhs2 = dot(r, r, n, red);
    int it = 0;
    double rr = rhs2;
    if (ok && rhs2 > 0.0) {
        cr_apply(r, z, na, cw);
        for (int w = tid; w < n; w += kPgoThreads) p[w] = z[w];
        __syncthreads();
        double rz = dot(r, z, n, red);
        const double stop2 = tol * tol * rhs2;
        while (it < max_iter) {
            spmv(H, rptr, col, lambda, p, q, na);
            const double alpha = rz / dot(p, q, n, red);
            for (int w = tid; w < n; w += kPgoThreads) { d[w] += alpha * p[w]; r[w] -= alpha * q[w]; }
            __syncthreads();
            rr = dot(r, r, n, red);
            ++it;
            if (!(rr > stop2)) break;                        // (a NaN residual stops too)
            cr_apply(r, z, na, cw);
            const double rz_new = dot(r, z, n, red);
            const double beta = rz_new / rz;
            rz = rz_new;
            for (int w = tid; w < n; w += kPgoThreads) p[w] = z[w] + beta * p[w];
            __syncthreads();
        }
    }
    double sc = 0.0;
    for (int w = tid; w < n; w += kPgoThreads) sc += d[w] * (lambda * d[w] - b[w]);
    sc = block_sum(sc, red);
    if (tid == 0) {
        scal[1] = (double)it;
        scal[2] = rhs2 > 0.0 ? sqrt(rr / rhs2) : 0.0;
        scal[3] = sc;
        scal[5] = ok ? 0.0 : 1.0;
    }
}

// trial[v] = est[v] * exp(d[act[v]]) for active v, a copy otherwise (d == nullptr: no update, score est itself);
// scal[out] = sum over edges of rho(e^T Omega e) (robust = 0: of e^T Omega e).
__global__ __launch_bounds__(kPgoThreads) void pgo_update_score_kernel(const double* __restrict__ est, double* __restrict__ trial,
                                                                       const int* __restrict__ act, int nv,
                                                                       const double* __restrict__ d, const int* __restrict__ ev,
                                                                       const double* __restrict__ meas,
                                                                       const double* __restrict__ info,
                                                                       const double* __restrict__ delta, int ne, int robust,
                                                                       double* __restrict__ scal, int out) {
    __shared__ double red[kPgoThreads];
    const int tid = threadIdx.x;
    const double* X = est;
    if (d) {
        for (int v = tid; v < nv; v += kPgoThreads) {
            const int a = act[v];
            if (a >= 0) {
                Iso Xv, Y;
                iso_load(est + (size_t)v * 16, Xv);
                iso_oplus(Xv, d + (size_t)a * 6, Y);
                iso_store(Y, trial + (size_t)v * 16);
            } else {
                for (int i = 0; i < 16; ++i) trial[(size_t)v * 16 + i] = est[(size_t)v * 16 + i];
            }
        }
        __syncthreads();
        X = trial;
    }
    double s = 0.0;
    for (int k = tid; k < ne; k += kPgoThreads) {
        Iso Xi, Xj, Z, Zinv;
        iso_load(X + (size_t)ev[2 * k] * 16, Xi);
        iso_load(X + (size_t)ev[2 * k + 1] * 16, Xj);
        iso_load(meas + (size_t)k * 16, Z);
        iso_inv(Z, Zinv);
        double e[6], rho, w;
        edge_error(Zinv, Xi, Xj, e);
        const double chi2 = quad_form(info + (size_t)k * 36, e);
        huber(chi2, robust ? delta[k] : 0.0, &rho, &w);
        s += rho;
    }
    s = block_sum(s, red);
    if (tid == 0) scal[out] = s;
}

__global__ __launch_bounds__(kPgoThreads) void pgo_max_diag_kernel(const double* __restrict__ H, const int* __restrict__ diag,
                                                                   int na, double* __restrict__ scal) {
    __shared__ double red[kPgoThreads];
    double m = 0.0;
    for (int w = threadIdx.x; w < 6 * na; w += kPgoThreads) {
        const int r = w / 6, c = w - r * 6;
        const double v = H[(size_t)diag[r] * 36 + c * 7];
        m = v > m ? v : m;
    }
    m = block_max(m, red);
    if (threadIdx.x == 0) scal[0] = m;
}

}  // namespace clslam

using namespace clslam;

extern "C" int clslam_pgo_edge_eval(const double* est, const int* edge_v, const double* meas, int ne, double* err, double* jac_i,
                                    double* jac_j, void* stream) {
    CLSLAM_REQUIRE(ne >= 0, "pgo_edge_eval: bad sizes");
    if (ne == 0) return CLSLAM_OK;
    CLSLAM_REQUIRE(est && edge_v && meas && err && jac_i && jac_j, "pgo_edge_eval: null");
    hipLaunchKernelGGL(pgo_edge_eval_kernel, dim3(cdiv(ne, 64)), dim3(64), 0, (hipStream_t)stream, est, edge_v, meas, ne, err,
                       jac_i, jac_j);
    return check_launch("pgo_edge_eval");
}

extern "C" int clslam_pgo_lin_stride(void) { return kLinStride; }

extern "C" int clslam_pgo_build_system(const double* est, const int* edge_v, const double* meas, const double* info,
                                       const double* huber_delta, int ne, const int* cptr, const int* contrib, const int* diag,
                                       int nnzb, int na, double* lin, double* H, double* b, double* scal, void* stream) {
    CLSLAM_REQUIRE(ne >= 1 && na >= 1 && nnzb >= na, "pgo_build_system: bad sizes");
    CLSLAM_REQUIRE(est && edge_v && meas && info && huber_delta && cptr && contrib && diag && lin && H && b && scal,
                   "pgo_build_system: null");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pgo_linearize_kernel, dim3(cdiv(ne, 64)), dim3(64), 0, st, est, edge_v, meas, info, huber_delta, ne, lin);
    int rc = check_launch("pgo_linearize");
    if (rc != CLSLAM_OK) return rc;
    hipLaunchKernelGGL(pgo_assemble_kernel, dim3(cdiv(nnzb + na, 256)), dim3(256), 0, st, (const double*)lin, cptr, contrib, diag,
                       nnzb, na, H, b);
    rc = check_launch("pgo_assemble");
    if (rc != CLSLAM_OK) return rc;
    hipLaunchKernelGGL(pgo_max_diag_kernel, dim3(1), dim3(kPgoThreads), 0, st, (const double*)H, diag, na, scal);
    return check_launch("pgo_max_diag");
}

extern "C" int clslam_pgo_solve_workspace(int na) { return na < 1 ? 0 : 30 * na + 4 * 36 * na + 72 * (na + 32); }

extern "C" int clslam_pgo_solve(const double* H, const int* rptr, const int* col, const int* tri, const double* b, double lambda,
                                int na, double tol, int max_iter, double* delta, double* work, double* scal, void* stream) {
    CLSLAM_REQUIRE(na >= 1 && max_iter >= 0 && lambda >= 0.0 && tol >= 0.0, "pgo_solve: bad arguments");
    CLSLAM_REQUIRE(H && rptr && col && tri && b && delta && work && scal, "pgo_solve: null");
    CrWork cw;
    double* vec = work;                                   // r z p q (+ spare): 5 * 6 na
    cw.A = work + 30 * (size_t)na;
    cw.B = cw.A + 36 * (size_t)na;
    cw.C = cw.B + 36 * (size_t)na;
    cw.Binv = cw.C + 36 * (size_t)na;
    cw.AG = cw.Binv + 36 * (size_t)na;                    // sum over levels of ceil(na / 2s) <= na + 32 records
    hipLaunchKernelGGL(pgo_solve_kernel, dim3(1), dim3(kPgoThreads), 0, (hipStream_t)stream, H, rptr, col, tri, b, lambda, na, tol,
                       max_iter, delta, vec, cw, scal);
    return check_launch("pgo_solve");
}

extern "C" int clslam_pgo_update_score(const double* est, double* trial, const int* act, int nv, const double* delta,
                                       const int* edge_v, const double* meas, const double* info, const double* huber_delta, int ne,
                                       int robust, double* scal, int out_index, void* stream) {
    CLSLAM_REQUIRE(nv >= 0 && ne >= 0 && out_index >= 0 && out_index < 8, "pgo_update_score: bad arguments");
    CLSLAM_REQUIRE(est && act && scal && (ne == 0 || (edge_v && meas && info && huber_delta)) && (!delta || trial),
                   "pgo_update_score: null");
    hipLaunchKernelGGL(pgo_update_score_kernel, dim3(1), dim3(kPgoThreads), 0, (hipStream_t)stream, est, trial, act, nv, delta,
                       edge_v, meas, info, huber_delta, ne, robust, scal, out_index);
    return check_launch("pgo_update_score");
}
