// PSLD SDE kernels: perturbation kernel p(z_t | x_0), HSM loss, Euler-Maruyama reverse step.
// Compiled with -ffp-contract=off so that the f32/f64 operation order of the reference's eager
// elementwise chains is reproduced without fused multiply-adds.
//
// Reference: main/models/sde/psld.py:38-44 (b_t, beta_t), :62-84 (_mean), :86-152 (_cov),
// :154-186 (get_coeff), :188-220 (get_inv_coeff), :230-260 (get_score), :262-287 (perturb_data),
// :330-364 (sde / reverse_sde); main/losses.py:94-130; main/samplers/sde.py:16-36.
// All public tensors here are NCHW like the reference ([B, 2C, H, W] state = [x | m]).
#include "common.h"
#include "psld_hip.h"

namespace {

constexpr int COEFF_STRIDE = 12;

#define GRID_STRIDE(i, n) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

inline int grid_for(long long n) {
    long long b = (n + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}

// psld.py:86-152 with the numerical_eps of :152 on the diagonal
__device__ void psld_cov(const psld_sde_params_t& p, double xx_0, double mm_0, double b, double& xx, double& xm,
                         double& mm) {
    const double nu = p.nu, ga = p.gamma, mi = p.m_inv, m = 1.0 / p.m_inv;
    const double lam = (nu + ga) / 2;
    const double b2 = b * b;
    const double sc = exp(-lam * b), isc = exp(lam * b);
    xx = (mi / 4 * b2 * xx_0 + mi * mi / 4 * b2 * mm_0 + (nu - ga) / 2 * b * xx_0 + (-mi / 2) * b2 +
          (ga - nu) / 2 * b + (isc - 1) + xx_0) * sc + p.numerical_eps;
    xm = ((ga - nu) / 8 * b2 * xx_0 + mi * (ga - nu) / 8 * b2 * mm_0 + (-1.0 / 2) * b * xx_0 + mi / 2 * b * mm_0 +
          (nu - ga) / 4 * b2) * sc;
    mm = (1.0 / 4 * b2 * xx_0 + mi / 4 * b2 * mm_0 + (ga - nu) / 2 * b * mm_0 + (-1.0 / 2) * b2 +
          m * (nu - ga) / 2 * b + m * (isc - 1) + mm_0) * sc + p.numerical_eps;
}

__global__ void perturb_coeffs_kernel(const double* __restrict__ t, int batch, const psld_sde_params_t p,
                                      double xx_0, double mm_0, double* __restrict__ out, int* __restrict__ nan_flag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    const double tt = t[i];
    const double b = p.beta_0 * tt + 0.5 * (tt * tt) * (p.beta_1 - p.beta_0);  // psld.py:42-44
    const double sf = exp(-((p.nu + p.gamma) / 4) * b);                        // psld.py:65-67
    double xx, xm, mm;
    psld_cov(p, xx_0, mm_0, b, xx, xm, mm);
    double c11, c12, c21, c22;
    if (p.decomp_lower) {  // psld.py:160-164
        c11 = sqrt(xx);
        c12 = 0.0;
        c21 = xm / c11;
        c22 = sqrt(mm - c21 * c21);
    } else {  // psld.py:174-178
        c22 = sqrt(mm);
        c12 = xm / c22;
        c11 = sqrt(xx - c12 * c12);
        c21 = 0.0;
    }
    if (isnan(c11) || isnan(c12) || isnan(c21) || isnan(c22)) atomicExch(nan_flag, 1);
    double* o = out + (long long)i * COEFF_STRIDE;
    o[0] = b; o[1] = sf; o[2] = 0; o[3] = 0;
    o[4] = c11; o[5] = c12; o[6] = c21; o[7] = c22;
    o[8] = xx; o[9] = xm; o[10] = mm; o[11] = 0;
}

// one thread per FOUR consecutive pixels of one (b, c) plane of the x half (hw % 4 == 0: 16-byte accesses); writes
// both halves.  VEC = 1 is the element-wise form for odd plane sizes.
template <int VEC>
__global__ void perturb_kernel(const float* __restrict__ x0, const float* __restrict__ m0,
                               const float* __restrict__ eps, const double* __restrict__ coeffs,
                               const psld_sde_params_t p, int batch, int c, int hw, float* __restrict__ z,
                               double* __restrict__ u, double* __restrict__ mu_out) {
    typedef float fv __attribute__((ext_vector_type(VEC)));
    typedef double dv __attribute__((ext_vector_type(VEC)));
    const long long n = (long long)batch * c * hw / VEC;
    const long long plane = (long long)c * hw / VEC;
    const double A1 = (p.nu - p.gamma) / 4, A2 = (p.gamma - p.nu) * (p.gamma - p.nu) / 8;
    const double C1 = -0.5, C2 = (p.gamma - p.nu) / 4;
    GRID_STRIDE(i, n) {
        const int b = (int)(i / plane);
        const long long r = i - (long long)b * plane;  // offset inside the half (in VEC units)
        const double* k = coeffs + (long long)b * COEFF_STRIDE;
        const double bt = k[0], sf = k[1];
        const fv xf = reinterpret_cast<const fv*>(x0)[i];
        fv mf = 0.f;
        if (m0) mf = reinterpret_cast<const fv*>(m0)[i];
        const long long ox = (long long)b * 2 * plane + r, om = ox + plane;
        const fv exf = reinterpret_cast<const fv*>(eps)[ox], emf = reinterpret_cast<const fv*>(eps)[om];
        fv zx, zm;
        dv ux, um, mx, mm;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const double xv = (double)xf[e], mv = (double)mf[e];
            // psld.py:76-83
            const double mu_x = (A1 * xv * bt + A2 * mv * bt + xv) * sf;
            const double mu_m = (C1 * xv * bt + C2 * mv * bt + mv) * sf;
            const double ex = (double)exf[e], em = (double)emf[e];
            // psld.py:277-283
            const double nx = k[4] * ex + k[5] * em;
            const double nm = k[6] * ex + k[7] * em;
            ux[e] = mu_x + nx; um[e] = mu_m + nm;
            mx[e] = mu_x; mm[e] = mu_m;
            zx[e] = (float)ux[e]; zm[e] = (float)um[e];
        }
        if (z) { reinterpret_cast<fv*>(z)[ox] = zx; reinterpret_cast<fv*>(z)[om] = zm; }
        if (u) { reinterpret_cast<dv*>(u)[ox] = ux; reinterpret_cast<dv*>(u)[om] = um; }
        if (mu_out) { reinterpret_cast<dv*>(mu_out)[ox] = mx; reinterpret_cast<dv*>(mu_out)[om] = mm; }
    }
}

// ---- loss ---------------------------------------------------------------------------------------
__global__ void sqerr_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, long long n,
                                     double* __restrict__ part, float* __restrict__ grad, float gscale) {
    __shared__ double red[4];
    double acc = 0.0;
    float local = 0.f;
    int cnt = 0;
    // 16 bytes per lane (n4 float4 items), then the < 4 leftover elements
    const long long n4 = n >> 2;
    GRID_STRIDE(i, n4) {
        const f32x4 va = reinterpret_cast<const f32x4*>(a)[i], vb = reinterpret_cast<const f32x4*>(b)[i];
        const f32x4 d = va - vb;
        local += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
        if (grad) reinterpret_cast<f32x4*>(grad)[i] = d * (-gscale);   // d/d(b) of (a-b)^2 * (gscale/2)
        if (++cnt == 4) { acc += (double)local; local = 0.f; cnt = 0; }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n & 3)) {
        const long long i = (n4 << 2) + threadIdx.x;
        const float d = a[i] - b[i];
        local += d * d;
        if (grad) grad[i] = -gscale * d;
    }
    acc += (double)local;
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void sqerr_final_kernel(const double* __restrict__ part, int nparts, double denom, float* __restrict__ loss) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) acc += part[i];
    acc = wave_sum_d(acc);
    if (threadIdx.x == 0) loss[0] = (float)(acc / denom);
}

// ---- reverse SDE / Euler-Maruyama ---------------------------------------------------------------
struct RevOut {
    double fbx, fbm, gx, gm;
};

__device__ __forceinline__ RevOut reverse_terms(const psld_em_coeffs_t& k, double xv, double mv, float ex, float em,
                                                bool have_ex) {
    // psld.py:336-337 drift, :339-340 diffusion
    const double fx = 0.5 * k.beta * (k.m_inv * mv - k.gamma * xv);
    const double fm = 0.5 * k.beta * (-k.nu * mv - xv);
    const double gx = sqrt(k.beta * k.gamma);
    const double gm = sqrt(k.beta * k.m * k.nu);
    // psld.py:240-259 score in f32 with f32-cast coefficients
    float sx, sm;
    if (k.score_mode == 1) {         // score_m, lower: eps is the momentum part only
        sx = 0.f;
        sm = -k.c22 * em;
    } else if (k.score_mode == 2) {  // score_x, upper
        sx = -k.c11 * ex;
        sm = 0.f;
    } else {
        sx = -k.c11 * ex - k.c12 * em;
        sm = -k.c21 * ex - k.c22 * em;
    }
    (void)have_ex;
    if (k.probability_flow) { sx = 0.5f * sx; sm = 0.5f * sm; }
    RevOut o;
    o.fbx = -fx + (gx * gx) * (double)sx;   // psld.py:360
    o.fbm = -fm + (gm * gm) * (double)sm;
    o.gx = k.probability_flow ? 0.0 : gx;
    o.gm = k.probability_flow ? 0.0 : gm;
    return o;
}

__device__ __forceinline__ void fetch_eps(const float* eps, const psld_em_coeffs_t& k, int b, long long r, int c, int hw,
                                          float& ex, float& em) {
    if (k.score_mode == 0) {
        const long long o = (long long)b * 2 * c * hw + r;
        ex = eps[o];
        em = eps[o + (long long)c * hw];
    } else {
        const float v = eps[(long long)b * c * hw + r];
        ex = v;
        em = v;
    }
}

__global__ void em_step_kernel(double* __restrict__ x, const float* __restrict__ eps, const double* __restrict__ z,
                               const psld_em_coeffs_t k, int batch, int c, int hw, float* __restrict__ xf) {
    const long long n = (long long)batch * c * hw;
    const double sdt = sqrt(k.dt);
    GRID_STRIDE(i, n) {
        const int b = (int)(i / ((long long)c * hw));
        const long long r = i - (long long)b * c * hw;
        const long long ox = (long long)b * 2 * c * hw + r, om = ox + (long long)c * hw;
        float ex, em;
        fetch_eps(eps, k, b, r, c, hw, ex, em);
        const double xv = x[ox], mv = x[om];
        const RevOut o = reverse_terms(k, xv, mv, ex, em, true);
        double nx = xv + o.fbx * k.dt;   // samplers/sde.py:23
        double nm = mv + o.fbm * k.dt;
        if (z) {                          // samplers/sde.py:24-25
            nx = nx + o.gx * sdt * z[ox];
            nm = nm + o.gm * sdt * z[om];
        }
        x[ox] = nx;
        x[om] = nm;
        if (xf) { xf[ox] = (float)nx; xf[om] = (float)nm; }
    }
}

__global__ void reverse_sde_kernel(const double* __restrict__ x, const float* __restrict__ eps,
                                   const psld_em_coeffs_t k, int batch, int c, int hw, double* __restrict__ fbar,
                                   double* __restrict__ gbar) {
    const long long n = (long long)batch * c * hw;
    GRID_STRIDE(i, n) {
        const int b = (int)(i / ((long long)c * hw));
        const long long r = i - (long long)b * c * hw;
        const long long ox = (long long)b * 2 * c * hw + r, om = ox + (long long)c * hw;
        float ex, em;
        fetch_eps(eps, k, b, r, c, hw, ex, em);
        const RevOut o = reverse_terms(k, x[ox], x[om], ex, em, true);
        fbar[ox] = o.fbx; fbar[om] = o.fbm;
        if (gbar) { gbar[ox] = o.gx; gbar[om] = o.gm; }
    }
}

// Per-sample times (psld.py:330-364 take t[B]): every thread derives its sample's scalars from t[b] on the device -
// no host read of t.  beta_t (psld.py:38-40), _cov (:86-152) and get_inv_coeff (:188-220) in f64, the inverse
// coefficients cast to f32 before they touch eps (:253-258) exactly like the one-time path's host scalars.
__global__ void reverse_sde_rows_kernel(const double* __restrict__ x, const float* __restrict__ eps,
                                        const double* __restrict__ t_rev, const psld_sde_params_t p, double xx_0,
                                        double mm_0, int score_mode, int probability_flow, int forward_only,
                                        int c, int hw, double* __restrict__ fbar, double* __restrict__ gbar,
                                        int* __restrict__ nan_flag) {
    const int b = blockIdx.y;
    const double tt = t_rev[b];
    psld_em_coeffs_t k;
    k.beta = p.beta_0 + tt * (p.beta_1 - p.beta_0);
    k.m_inv = p.m_inv; k.gamma = p.gamma; k.nu = p.nu; k.m = 1.0 / p.m_inv;
    k.dt = 0.0; k.score_mode = score_mode; k.probability_flow = probability_flow;
    k.c11 = k.c12 = k.c21 = k.c22 = 0.f;
    if (!forward_only) {
        const double bt = p.beta_0 * tt + 0.5 * (tt * tt) * (p.beta_1 - p.beta_0);
        double xx, xm, mm;
        psld_cov(p, xx_0, mm_0, bt, xx, xm, mm);
        const double det = xx * mm - xm * xm;
        double c11, c12, c21, c22;
        if (p.decomp_lower) {   // psld.py:194-199
            c11 = sqrt(1 / xx); c12 = -xm / (sqrt(xx) * sqrt(det)); c21 = 0.0; c22 = sqrt(xx / det);
        } else {                // psld.py:207-212
            c11 = sqrt(mm / det); c12 = 0.0; c21 = -xm / (sqrt(mm) * sqrt(det)); c22 = sqrt(1 / mm);
        }
        if ((isnan(c11) || isnan(c12) || isnan(c21) || isnan(c22)) && threadIdx.x == 0 && blockIdx.x == 0)
            atomicExch(nan_flag, 1);
        k.c11 = (float)c11; k.c12 = (float)c12; k.c21 = (float)c21; k.c22 = (float)c22;
    }
    const long long n = (long long)c * hw;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long long)gridDim.x * blockDim.x) {
        const long long ox = (long long)b * 2 * c * hw + r, om = ox + (long long)c * hw;
        float ex = 0.f, em = 0.f;
        if (!forward_only) fetch_eps(eps, k, b, r, c, hw, ex, em);
        const RevOut o = reverse_terms(k, x[ox], x[om], ex, em, true);
        if (forward_only) {     // sde(): (f, g) themselves; -(-f + 0) is exact
            fbar[ox] = -o.fbx; fbar[om] = -o.fbm;
        } else {
            fbar[ox] = o.fbx; fbar[om] = o.fbm;
        }
        if (gbar) { gbar[ox] = o.gx; gbar[om] = o.gm; }
    }
}

// ---- symmetric-splitting sampler (samplers/sde.py:227-370) ----------------------------------------
// analytic half step: u' = M u + L z with host-computed 2x2 mean matrix (incl. exp scaling) and
// Cholesky factor of the transition covariance (sde.py:236-311)
__global__ void sscs_analytic_kernel(double* __restrict__ x, const double* __restrict__ z, const psld_sscs_coeffs_t k,
                                     int batch, int c, int hw, float* __restrict__ xf) {
    const long long n = (long long)batch * c * hw;
    GRID_STRIDE(i, n) {
        const int b = (int)(i / ((long long)c * hw));
        const long long r = i - (long long)b * c * hw;
        const long long ox = (long long)b * 2 * c * hw + r, om = ox + (long long)c * hw;
        const double xv = x[ox], mv = x[om];
        const double zx = z[ox], zm = z[om];
        const double nx = (k.a_xx * xv + k.a_xm * mv) + (k.c11 * zx + k.c12 * zm);
        const double nm = (k.a_mx * xv + k.a_mm * mv) + (k.c21 * zx + k.c22 * zm);
        x[ox] = nx;
        x[om] = nm;
        if (xf) { xf[ox] = (float)nx; xf[om] = (float)nm; }
    }
}

// score step (sde.py:313-329): x += dt*gamma*beta*(score_x + x);  m += dt*m*nu*beta*(score_m + m_inv*m)
__global__ void sscs_score_kernel(double* __restrict__ x, const float* __restrict__ eps, const psld_em_coeffs_t k,
                                  int batch, int c, int hw) {
    const long long n = (long long)batch * c * hw;
    GRID_STRIDE(i, n) {
        const int b = (int)(i / ((long long)c * hw));
        const long long r = i - (long long)b * c * hw;
        const long long ox = (long long)b * 2 * c * hw + r, om = ox + (long long)c * hw;
        float ex, em;
        fetch_eps(eps, k, b, r, c, hw, ex, em);
        float sx, sm;
        if (k.score_mode == 1) { sx = 0.f; sm = -k.c22 * em; }
        else if (k.score_mode == 2) { sx = -k.c11 * ex; sm = 0.f; }
        else { sx = -k.c11 * ex - k.c12 * em; sm = -k.c21 * ex - k.c22 * em; }
        const double xv = x[ox], mv = x[om];
        x[ox] = xv + k.dt * k.gamma * k.beta * ((double)sx + xv);
        x[om] = mv + k.dt * k.m * k.nu * k.beta * ((double)sm + k.m_inv * mv);
    }
}

// ---- exponential-integrator sampler (no counterpart in the reference) -----------
// u' = Phi u + sum_j C_j eps_j: host-computed float64 2x2 matrices (augmented) or scalars (VP-SDE), up to three float32
// eps buffers promoted to double.  VEC = 4: one thread per four consecutive elements of a segment - 16-byte accesses on
// the float64 state (two per half), the float32 eps and the float32 copy; VEC = 1 is the element-wise form.  A segment
// is one sample's x half (augmented; the m half lies `seg` elements behind it) or the whole flat state.
struct EiArgs {
    const float* e[3];
};

template <int VEC>
__device__ __forceinline__ void ei_load(const double* p, double (&v)[VEC]) {
    if constexpr (VEC == 4) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        const d2 a = reinterpret_cast<const d2*>(p)[0], b = reinterpret_cast<const d2*>(p)[1];
        v[0] = a[0]; v[1] = a[1]; v[2] = b[0]; v[3] = b[1];
    } else {
        v[0] = p[0];
    }
}
template <int VEC>
__device__ __forceinline__ void ei_load(const float* p, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        typedef float f4 __attribute__((ext_vector_type(4)));
        const f4 a = reinterpret_cast<const f4*>(p)[0];
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    } else {
        v[0] = p[0];
    }
}
template <int VEC>
__device__ __forceinline__ void ei_store(double* p, float* pf, const double (&v)[VEC]) {
    if constexpr (VEC == 4) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        typedef float f4 __attribute__((ext_vector_type(4)));
        d2 a, b;
        a[0] = v[0]; a[1] = v[1]; b[0] = v[2]; b[1] = v[3];
        reinterpret_cast<d2*>(p)[0] = a;
        reinterpret_cast<d2*>(p)[1] = b;
        if (pf) {
            f4 f;
            f[0] = (float)v[0]; f[1] = (float)v[1]; f[2] = (float)v[2]; f[3] = (float)v[3];
            reinterpret_cast<f4*>(pf)[0] = f;
        }
    } else {
        p[0] = v[0];
        if (pf) pf[0] = (float)v[0];
    }
}

// VEC elements at element offset ox (and om = the momentum half, augmented only)
template <int VEC, bool AUG>
__device__ __forceinline__ void ei_update(double* __restrict__ x, const EiArgs& a, const psld_ei_coeffs_t& k,
                                          long long ox, long long om, float* __restrict__ xf) {
    double xv[VEC], mv[VEC], nx[VEC], nm[VEC];
    ei_load<VEC>(x + ox, xv);
    if constexpr (AUG) ei_load<VEC>(x + om, mv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        if constexpr (AUG) {
            nx[e] = k.phi[0] * xv[e] + k.phi[1] * mv[e];
            nm[e] = k.phi[2] * xv[e] + k.phi[3] * mv[e];
        } else {
            nx[e] = k.phi[0] * xv[e];
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j < k.n_hist) {
            float ex[VEC], em[VEC];
            ei_load<VEC>(a.e[j] + ox, ex);
            if constexpr (AUG) ei_load<VEC>(a.e[j] + om, em);
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                if constexpr (AUG) {
                    nx[e] = nx[e] + (k.c[j][0] * (double)ex[e] + k.c[j][1] * (double)em[e]);
                    nm[e] = nm[e] + (k.c[j][2] * (double)ex[e] + k.c[j][3] * (double)em[e]);
                } else {
                    nx[e] = nx[e] + k.c[j][0] * (double)ex[e];
                }
            }
        }
    }
    ei_store<VEC>(x + ox, xf ? xf + ox : nullptr, nx);
    if constexpr (AUG) ei_store<VEC>(x + om, xf ? xf + om : nullptr, nm);
}

// nseg segments of `seg` elements; segment s starts at element s * stride.  The first seg / VEC * VEC elements of every
// segment go VEC at a time, the rest (only where VEC = 4 and seg % 4 != 0: the flat VP-SDE state) one at a time.
template <int VEC, bool AUG>
__global__ void ei_step_kernel(double* __restrict__ x, const EiArgs a, const psld_ei_coeffs_t k, long long nseg,
                               long long seg, long long stride, float* __restrict__ xf) {
    const long long pv = seg / VEC, nvec = nseg * pv;
    GRID_STRIDE(i, nvec) {
        const long long s = i / pv, r = (i - s * pv) * VEC;
        const long long ox = s * stride + r;
        ei_update<VEC, AUG>(x, a, k, ox, ox + seg, xf);
    }
    if constexpr (VEC > 1) {
        const long long tail = seg - pv * VEC, ntail = nseg * tail;
        GRID_STRIDE(i, ntail) {
            const long long s = i / tail, r = pv * VEC + (i - s * tail);
            const long long ox = s * stride + r;
            ei_update<1, AUG>(x, a, k, ox, ox + seg, xf);
        }
    }
}

// The stochastic member (ei_sde): u' = Phi u + C eps + S z with one eps buffer and float64 noise in the
// state's layout, S lower-triangular.  Same segments, same accesses and, for the terms it shares with ei_update at
// n_hist = 1, the same order of operations; the noise goes on last.
template <int VEC, bool AUG>
__device__ __forceinline__ void ei_sde_update(double* __restrict__ x, const float* __restrict__ eps,
                                              const double* __restrict__ z, const psld_ei_sde_coeffs_t& k, long long ox,
                                              long long om, float* __restrict__ xf) {
    double xv[VEC], mv[VEC], zx[VEC], zm[VEC], nx[VEC], nm[VEC];
    float ex[VEC], em[VEC];
    ei_load<VEC>(x + ox, xv);
    ei_load<VEC>(eps + ox, ex);
    ei_load<VEC>(z + ox, zx);
    if constexpr (AUG) {
        ei_load<VEC>(x + om, mv);
        ei_load<VEC>(eps + om, em);
        ei_load<VEC>(z + om, zm);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        if constexpr (AUG) {
            nx[e] = k.phi[0] * xv[e] + k.phi[1] * mv[e];
            nm[e] = k.phi[2] * xv[e] + k.phi[3] * mv[e];
            nx[e] = nx[e] + (k.c[0] * (double)ex[e] + k.c[1] * (double)em[e]);
            nm[e] = nm[e] + (k.c[2] * (double)ex[e] + k.c[3] * (double)em[e]);
            nx[e] = nx[e] + k.s[0] * zx[e];
            nm[e] = nm[e] + (k.s[2] * zx[e] + k.s[3] * zm[e]);
        } else {
            nx[e] = k.phi[0] * xv[e];
            nx[e] = nx[e] + k.c[0] * (double)ex[e];
            nx[e] = nx[e] + k.s[0] * zx[e];
        }
    }
    ei_store<VEC>(x + ox, xf ? xf + ox : nullptr, nx);
    if constexpr (AUG) ei_store<VEC>(x + om, xf ? xf + om : nullptr, nm);
}

// the segments of ei_step_kernel
template <int VEC, bool AUG>
__global__ void ei_sde_step_kernel(double* __restrict__ x, const float* __restrict__ eps, const double* __restrict__ z,
                                   const psld_ei_sde_coeffs_t k, long long nseg, long long seg, long long stride,
                                   float* __restrict__ xf) {
    const long long pv = seg / VEC, nvec = nseg * pv;
    GRID_STRIDE(i, nvec) {
        const long long s = i / pv, r = (i - s * pv) * VEC;
        const long long ox = s * stride + r;
        ei_sde_update<VEC, AUG>(x, eps, z, k, ox, ox + seg, xf);
    }
    if constexpr (VEC > 1) {
        const long long tail = seg - pv * VEC, ntail = nseg * tail;
        GRID_STRIDE(i, ntail) {
            const long long s = i / tail, r = pv * VEC + (i - s * tail);
            const long long ox = s * stride + r;
            ei_sde_update<1, AUG>(x, eps, z, k, ox, ox + seg, xf);
        }
    }
}

// ---- adaptive RK45 building blocks (black-box probability-flow ODE sampler, samplers/ode.py) ---------
struct RkArgs {
    const double* v[8];
    double c[8];
    int nv;
};
// out = base + sum_j c_j v_j  (base may be null); optional f32 copy for the next network call
__global__ void rk_lincomb_kernel(double* __restrict__ out, const double* __restrict__ base, const RkArgs a,
                                  long long n, float* __restrict__ out32) {
    GRID_STRIDE(i, n) {
        double acc = base ? base[i] : 0.0;
#pragma unroll 8
        for (int j = 0; j < a.nv; ++j) acc += a.c[j] * a.v[j][i];
        out[i] = acc;
        if (out32) out32[i] = (float)acc;
    }
}
// partial sums of ((sum_j c_j v_j) / (atol + rtol * max(|p|,|q|)))^2
__global__ void rk_scaled_sq_kernel(const RkArgs a, const double* __restrict__ p, const double* __restrict__ q,
                                    double atol, double rtol, long long n, double* __restrict__ part) {
    __shared__ double red[4];
    double acc = 0.0;
    GRID_STRIDE(i, n) {
        double e = 0.0;
#pragma unroll 8
        for (int j = 0; j < a.nv; ++j) e += a.c[j] * a.v[j][i];
        const double sc = atol + rtol * fmax(fabs(p[i]), fabs(q[i]));
        const double r = e / sc;
        acc += r * r;
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void rk_final_kernel(const double* __restrict__ part, int nparts, double* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) acc += part[i];
    acc = wave_sum_d(acc);
    if (threadIdx.x == 0) out[0] = acc;
}

// ---- VP-SDE baseline (main/models/sde/vpsde.py) ---------------------------------------------------
// x_t = exp(lmc) * x0 + sqrt(1 - exp(2 lmc)) * eps, lmc = -0.25 t^2 (b1-b0) - 0.5 t b0   (vpsde.py:29-37, 72-83)
__global__ void vp_perturb_kernel(const float* __restrict__ x0, const float* __restrict__ eps,
                                  const double* __restrict__ t, double beta0, double beta1, int batch, long long per,
                                  float* __restrict__ z, double* __restrict__ u) {
    const long long n = (long long)batch * per;
    GRID_STRIDE(i, n) {
        const int b = (int)(i / per);
        const double tt = t[b];
        const double lmc = -0.25 * (tt * tt) * (beta1 - beta0) - 0.5 * tt * beta0;
        const double mean = exp(lmc) * (double)x0[i];
        const double sd = sqrt(1.0 - exp(2.0 * lmc));
        const double v = mean + (double)eps[i] * sd;
        if (z) z[i] = (float)v;
        if (u) u[i] = v;
    }
}
// reverse drift f_bar = 0.5 beta x + beta * score, score = -eps/std (f64), x0.5 for probability flow
// (vpsde.py:26-27, 39-66); mode 0: write f_bar (and g_bar), mode 1: Euler-Maruyama update of x in place
__global__ void vp_reverse_kernel(double* __restrict__ x, const float* __restrict__ eps, const double* __restrict__ z,
                                  double beta, double sd, double dt, int pf, int mode, long long n,
                                  double* __restrict__ fbar, float* __restrict__ xf) {
    const double g = sqrt(beta);
    const double sdt = sqrt(dt);
    GRID_STRIDE(i, n) {
        const double xv = x[i];
        double score = -(double)eps[i] / sd;
        if (pf) score = 0.5 * score;
        const double fb = -(-0.5 * beta * xv) + (g * g) * score;
        if (mode == 0) {
            fbar[i] = fb;
        } else {
            double nx = xv + fb * dt;
            if (z) nx = nx + g * sdt * z[i];
            x[i] = nx;
            if (xf) xf[i] = (float)nx;
        }
    }
}

}  // namespace

extern "C" int psld_vp_perturb_f32(const float* x0, const float* eps, const double* t, double beta0, double beta1,
                                   int batch, long long per_image, float* z_f32, double* u_f64, hipStream_t stream) {
    PSLD_CHECK_ARG(x0 && eps && t && batch > 0 && per_image > 0 && (z_f32 || u_f64), "psld_vp_perturb_f32: bad args");
    hipLaunchKernelGGL(vp_perturb_kernel, dim3(grid_for((long long)batch * per_image)), dim3(256), 0, stream, x0, eps, t,
                       beta0, beta1, batch, per_image, z_f32, u_f64);
    PSLD_CHECK_LAUNCH("psld_vp_perturb_f32");
    return PSLD_OK;
}

extern "C" int psld_vp_reverse_f64(double* x, const float* eps_pred, const double* z, double beta, double std, double dt,
                                   int probability_flow, int mode, long long n, double* f_bar, float* x_f32_out,
                                   hipStream_t stream) {
    PSLD_CHECK_ARG(x && eps_pred && n > 0 && (mode == 1 || f_bar), "psld_vp_reverse_f64: bad args");
    hipLaunchKernelGGL(vp_reverse_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x, eps_pred, z, beta, std, dt,
                       probability_flow, mode, n, f_bar, x_f32_out);
    PSLD_CHECK_LAUNCH("psld_vp_reverse_f64");
    return PSLD_OK;
}

// x <- x*(1 - mask) + u*mask on both halves [x | m] of the state (samplers/sde.py:170-174): mask is {0, 1}, so this
// selects; the reference's arithmetic form is kept (built with -ffp-contract=off) to stay bit-identical with it.
__global__ void mask_combine_kernel(double* __restrict__ x, const double* __restrict__ u, const float* __restrict__ mask,
                                    long long per_img, long long total, float* __restrict__ x_f32) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long img = i / (2 * per_img), r = i - img * 2 * per_img;
        const double m = (double)mask[img * per_img + (r < per_img ? r : r - per_img)];
        const double v = x[i] * (1.0 - m) + u[i] * m;
        x[i] = v;
        if (x_f32) x_f32[i] = (float)v;
    }
}

// Classifier guidance (samplers/sde.py:90-94): adding g^2 * grad to the drift moves the state by g^2 * grad * dt;
// g^2 differs between the position and momentum halves (psld.py:201-203), so one coefficient per half.
__global__ void guide_kernel(double* __restrict__ x, const float* __restrict__ grad, double cx, double cm,
                             long long per_img, long long total, float* __restrict__ x_f32) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long r = i % (2 * per_img);
        const double v = x[i] + (r < per_img ? cx : cm) * (double)grad[i];
        x[i] = v;
        if (x_f32) x_f32[i] = (float)v;
    }
}

extern "C" int psld_guide_f64(double* x, const float* grad, double coef_x, double coef_m, int batch, int c, int hw,
                              float* x_f32_out, hipStream_t stream) {
    PSLD_CHECK_ARG(x && grad && batch > 0 && c > 0 && hw > 0, "psld_guide_f64: bad args");
    const long long per_img = (long long)c * hw, total = 2 * per_img * batch;
    hipLaunchKernelGGL(guide_kernel, dim3(grid_for(total)), dim3(256), 0, stream, x, grad, coef_x, coef_m, per_img, total,
                       x_f32_out);
    PSLD_CHECK_LAUNCH("psld_guide_f64");
    return PSLD_OK;
}

extern "C" int psld_mask_combine_f64(double* x, const double* u, const float* mask, int batch, int c, int hw,
                                     float* x_f32_out, hipStream_t stream) {
    PSLD_CHECK_ARG(x && u && mask && batch > 0 && c > 0 && hw > 0, "psld_mask_combine_f64: bad args");
    const long long per_img = (long long)c * hw, total = 2 * per_img * batch;
    hipLaunchKernelGGL(mask_combine_kernel, dim3(grid_for(total)), dim3(256), 0, stream, x, u, mask, per_img, total,
                       x_f32_out);
    PSLD_CHECK_LAUNCH("psld_mask_combine_f64");
    return PSLD_OK;
}

extern "C" int psld_lincomb_f64(double* out, const double* base, const double* const* v, const double* coef, int nv,
                                long long n, float* out_f32, hipStream_t stream) {
    PSLD_CHECK_ARG(out && v && coef && nv >= 0 && nv <= 8 && n > 0, "psld_lincomb_f64: bad args");
    RkArgs a{};
    a.nv = nv;
    for (int j = 0; j < nv; ++j) { a.v[j] = v[j]; a.c[j] = coef[j]; }
    hipLaunchKernelGGL(rk_lincomb_kernel, dim3(grid_for(n)), dim3(256), 0, stream, out, base, a, n, out_f32);
    PSLD_CHECK_LAUNCH("psld_lincomb_f64");
    return PSLD_OK;
}

extern "C" int psld_scaled_norm_sq_f64(const double* const* v, const double* coef, int nv, const double* p,
                                       const double* q, double atol, double rtol, long long n, double* out,
                                       void* workspace, hipStream_t stream) {
    PSLD_CHECK_ARG(v && coef && nv >= 1 && nv <= 8 && p && q && out && workspace && n > 0,
                   "psld_scaled_norm_sq_f64: bad args");
    RkArgs a{};
    a.nv = nv;
    for (int j = 0; j < nv; ++j) { a.v[j] = v[j]; a.c[j] = coef[j]; }
    const int blocks = grid_for(n);
    double* part = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(rk_scaled_sq_kernel, dim3(blocks), dim3(256), 0, stream, a, p, q, atol, rtol, n, part);
    PSLD_CHECK_LAUNCH("rk_scaled_sq_kernel");
    hipLaunchKernelGGL(rk_final_kernel, dim3(1), dim3(64), 0, stream, part, blocks, out);
    PSLD_CHECK_LAUNCH("rk_final_kernel");
    return PSLD_OK;
}

extern "C" int psld_sscs_analytic_f64(double* x, const double* z, const psld_sscs_coeffs_t* k, int batch, int c,
                                      int hw, float* x_f32_out, hipStream_t stream) {
    PSLD_CHECK_ARG(x && z && k && batch > 0 && c > 0 && hw > 0, "psld_sscs_analytic_f64: bad args");
    const long long n = (long long)batch * c * hw;
    hipLaunchKernelGGL(sscs_analytic_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x, z, *k, batch, c, hw,
                       x_f32_out);
    PSLD_CHECK_LAUNCH("psld_sscs_analytic_f64");
    return PSLD_OK;
}

extern "C" int psld_sscs_score_step_f64(double* x, const float* eps_pred, const psld_em_coeffs_t* k, int batch,
                                        int c, int hw, hipStream_t stream) {
    PSLD_CHECK_ARG(x && eps_pred && k && batch > 0 && c > 0 && hw > 0, "psld_sscs_score_step_f64: bad args");
    const long long n = (long long)batch * c * hw;
    hipLaunchKernelGGL(sscs_score_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x, eps_pred, *k, batch, c, hw);
    PSLD_CHECK_LAUNCH("psld_sscs_score_step_f64");
    return PSLD_OK;
}

extern "C" int psld_ei_step_f64(double* x, const float* const* eps, const psld_ei_coeffs_t* k, int batch, int c, int hw,
                                float* x_f32_out, hipStream_t stream) {
    PSLD_CHECK_ARG(x && eps && k && batch > 0 && c > 0 && hw > 0, "psld_ei_step_f64: bad args");
    PSLD_CHECK_ARG(k->n_hist >= 1 && k->n_hist <= 3 && (k->augmented == 0 || k->augmented == 1),
                   "psld_ei_step_f64: n_hist %d not in 1..3 or augmented %d not 0 / 1", k->n_hist, k->augmented);
    EiArgs a{};
    bool aligned = ((uintptr_t)x | (uintptr_t)x_f32_out) % 16 == 0;
    for (int j = 0; j < k->n_hist; ++j) {
        PSLD_CHECK_ARG(eps[j], "psld_ei_step_f64: eps[%d] is NULL", j);
        a.e[j] = eps[j];
        aligned = aligned && (uintptr_t)eps[j] % 16 == 0;
    }
    const long long plane = (long long)c * hw;
    if (k->augmented) {
        if (aligned && plane % 4 == 0)
            hipLaunchKernelGGL((ei_step_kernel<4, true>), dim3(grid_for(batch * plane / 4)), dim3(256), 0, stream, x, a,
                               *k, (long long)batch, plane, 2 * plane, x_f32_out);
        else
            hipLaunchKernelGGL((ei_step_kernel<1, true>), dim3(grid_for(batch * plane)), dim3(256), 0, stream, x, a, *k,
                               (long long)batch, plane, 2 * plane, x_f32_out);
    } else {
        const long long n = batch * plane;
        if (aligned && n >= 4)
            hipLaunchKernelGGL((ei_step_kernel<4, false>), dim3(grid_for(n / 4)), dim3(256), 0, stream, x, a, *k, 1LL, n,
                               n, x_f32_out);
        else
            hipLaunchKernelGGL((ei_step_kernel<1, false>), dim3(grid_for(n)), dim3(256), 0, stream, x, a, *k, 1LL, n, n,
                               x_f32_out);
    }
    PSLD_CHECK_LAUNCH("psld_ei_step_f64");
    return PSLD_OK;
}

extern "C" int psld_ei_sde_step_f64(double* x, const float* eps, const double* z, const psld_ei_sde_coeffs_t* k, int batch,
                                    int c, int hw, float* x_f32_out, hipStream_t stream) {
    PSLD_CHECK_ARG(x && eps && k && batch > 0 && c > 0 && hw > 0, "psld_ei_sde_step_f64: bad args");
    PSLD_CHECK_ARG(k->augmented == 0 || k->augmented == 1, "psld_ei_sde_step_f64: augmented %d not 0 / 1", k->augmented);
    if (!z) {   // no noise term: the deterministic kernel itself, on the same Phi and C
        psld_ei_coeffs_t d{};
        for (int i = 0; i < 4; ++i) { d.phi[i] = k->phi[i]; d.c[0][i] = k->c[i]; }
        d.n_hist = 1;
        d.augmented = k->augmented;
        const float* e[1] = {eps};
        return psld_ei_step_f64(x, e, &d, batch, c, hw, x_f32_out, stream);
    }
    const bool aligned = ((uintptr_t)x | (uintptr_t)eps | (uintptr_t)z | (uintptr_t)x_f32_out) % 16 == 0;
    const long long plane = (long long)c * hw;
    if (k->augmented) {
        if (aligned && plane % 4 == 0)
            hipLaunchKernelGGL((ei_sde_step_kernel<4, true>), dim3(grid_for(batch * plane / 4)), dim3(256), 0, stream, x, eps,
                               z, *k, (long long)batch, plane, 2 * plane, x_f32_out);
        else
            hipLaunchKernelGGL((ei_sde_step_kernel<1, true>), dim3(grid_for(batch * plane)), dim3(256), 0, stream, x, eps, z,
                               *k, (long long)batch, plane, 2 * plane, x_f32_out);
    } else {
        const long long n = batch * plane;
        if (aligned && n >= 4)
            hipLaunchKernelGGL((ei_sde_step_kernel<4, false>), dim3(grid_for(n / 4)), dim3(256), 0, stream, x, eps, z, *k, 1LL,
                               n, n, x_f32_out);
        else
            hipLaunchKernelGGL((ei_sde_step_kernel<1, false>), dim3(grid_for(n)), dim3(256), 0, stream, x, eps, z, *k, 1LL, n,
                               n, x_f32_out);
    }
    PSLD_CHECK_LAUNCH("psld_ei_sde_step_f64");
    return PSLD_OK;
}

extern "C" long long psld_reduce_workspace_bytes(long long n) {
    (void)n;
    return 4096LL * sizeof(double);
}

extern "C" int psld_perturb_coeffs_f64(const double* t, int batch, const psld_sde_params_t* p, double xx_0,
                                       double mm_0, double* coeffs, int* nan_flag, hipStream_t stream) {
    PSLD_CHECK_ARG(t && p && coeffs && nan_flag && batch > 0, "psld_perturb_coeffs_f64: bad args");
    hipLaunchKernelGGL(perturb_coeffs_kernel, dim3(cdiv(batch, 128)), dim3(128), 0, stream, t, batch, *p, xx_0, mm_0,
                       coeffs, nan_flag);
    PSLD_CHECK_LAUNCH("psld_perturb_coeffs_f64");
    return PSLD_OK;
}

extern "C" int psld_perturb_f32(const float* x0, const float* m0, const float* eps, const double* coeffs,
                                   const psld_sde_params_t* p, int batch, int c, int hw, float* z_f32, double* u_f64,
                                   double* mu_f64, hipStream_t stream) {
    PSLD_CHECK_ARG(x0 && eps && coeffs && p && batch > 0 && c > 0 && hw > 0, "psld_perturb_f32: bad args");
    const long long n = (long long)batch * c * hw;
    auto al = [](const void* q, uintptr_t a) { return q == nullptr || (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; };
    if (hw % 4 == 0 && al(x0, 16) && al(m0, 16) && al(eps, 16) && al(z_f32, 16) && al(u_f64, 32) && al(mu_f64, 32))
        hipLaunchKernelGGL(perturb_kernel<4>, dim3(grid_for(n / 4)), dim3(256), 0, stream, x0, m0, eps, coeffs, *p, batch, c,
                           hw, z_f32, u_f64, mu_f64);
    else
        hipLaunchKernelGGL(perturb_kernel<1>, dim3(grid_for(n)), dim3(256), 0, stream, x0, m0, eps, coeffs, *p, batch, c, hw,
                           z_f32, u_f64, mu_f64);
    PSLD_CHECK_LAUNCH("psld_perturb_f32");
    return PSLD_OK;
}

extern "C" int psld_sqerr_loss_f32(const float* eps, const float* eps_pred, long long n, int reduce_mean, float* loss,
                                   float* grad, float grad_scale, void* workspace, hipStream_t stream) {
    PSLD_CHECK_ARG(eps && eps_pred && loss && workspace && n > 0, "psld_sqerr_loss_f32: bad args");
    PSLD_CHECK_ARG(((reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(eps_pred) |
                     reinterpret_cast<uintptr_t>(grad)) & 15) == 0, "psld_sqerr_loss_f32: operands must be 16-byte aligned");
    int blocks = grid_for((n + 3) / 4);
    if (blocks > 4096) blocks = 4096;
    double* part = reinterpret_cast<double*>(workspace);
    // d loss / d eps_pred = 2*(pred - eps)/denom * upstream  ==  -(gscale) * (eps - pred)
    const double denom = reduce_mean ? (double)n : 1.0;
    const float gs = (float)(2.0 * (double)grad_scale / denom);
    hipLaunchKernelGGL(sqerr_partial_kernel, dim3(blocks), dim3(256), 0, stream, eps, eps_pred, n, part, grad, gs);
    PSLD_CHECK_LAUNCH("sqerr_partial_kernel");
    hipLaunchKernelGGL(sqerr_final_kernel, dim3(1), dim3(64), 0, stream, part, blocks, denom, loss);
    PSLD_CHECK_LAUNCH("sqerr_final_kernel");
    return PSLD_OK;
}

extern "C" int psld_em_step_f64(double* x, const float* eps_pred, const double* z, const psld_em_coeffs_t* k, int batch,
                                int c, int hw, float* x_f32_out, hipStream_t stream) {
    PSLD_CHECK_ARG(x && eps_pred && k && batch > 0 && c > 0 && hw > 0, "psld_em_step_f64: bad args");
    const long long n = (long long)batch * c * hw;
    hipLaunchKernelGGL(em_step_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x, eps_pred, z, *k, batch, c, hw,
                       x_f32_out);
    PSLD_CHECK_LAUNCH("psld_em_step_f64");
    return PSLD_OK;
}

extern "C" int psld_reverse_sde_f64(const double* x, const float* eps_pred, const psld_em_coeffs_t* k, int batch, int c,
                                    int hw, double* f_bar, double* g_bar, hipStream_t stream) {
    PSLD_CHECK_ARG(x && eps_pred && k && f_bar && batch > 0, "psld_reverse_sde_f64: bad args");
    const long long n = (long long)batch * c * hw;
    hipLaunchKernelGGL(reverse_sde_kernel, dim3(grid_for(n)), dim3(256), 0, stream, x, eps_pred, *k, batch, c, hw,
                       f_bar, g_bar);
    PSLD_CHECK_LAUNCH("psld_reverse_sde_f64");
    return PSLD_OK;
}

extern "C" int psld_reverse_sde_rows_f64(const double* x, const float* eps_pred, const double* t_rev,
                                         const psld_sde_params_t* p, double xx_0, double mm_0, int score_mode,
                                         int probability_flow, int batch, int c, int hw, double* f_bar, double* g_bar,
                                         int* nan_flag, hipStream_t stream) {
    PSLD_CHECK_ARG(x && t_rev && p && f_bar && nan_flag && batch > 0 && c > 0 && hw > 0 && batch <= 65535,
                   "psld_reverse_sde_rows_f64: bad args");
    const long long n = (long long)c * hw;
    int bx = (int)((n + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(reverse_sde_rows_kernel, dim3(bx, batch), dim3(256), 0, stream, x, eps_pred, t_rev, *p, xx_0, mm_0,
                       score_mode, probability_flow, eps_pred ? 0 : 1, c, hw, f_bar, g_bar, nan_flag);
    PSLD_CHECK_LAUNCH("psld_reverse_sde_rows_f64");
    return PSLD_OK;
}

// ---- ScoreLoss beyond the eps-MSE (main/losses.py:38-39, 55-63) --------------------------------------------
// mode 1: L1 criterion |eps - eps_pred| (f32 like nn.L1Loss); mode 2: 'nll' weighting, per element
// (score(eps_pred) - score(eps))^2 * g(t)^2 with score = -eps / std(t) (vpsde.py:26-27) and g(t)^2 = beta(t)
// (vpsde.py:97-99), evaluated in f64 like the reference (t is f64 there).
__global__ void vp_score_loss_kernel(const float* __restrict__ e, const float* __restrict__ ep,
                                     const double* __restrict__ t, double beta0, double beta1, long long per,
                                     long long n, int mode, double* __restrict__ part, float* __restrict__ grad,
                                     double gscale) {
    __shared__ double red[4];
    double acc = 0.0;
    GRID_STRIDE(i, n) {
        if (mode == 1) {
            const float d = e[i] - ep[i];
            acc += (double)fabsf(d);
            if (grad) grad[i] = (float)(gscale * (d > 0.f ? -1.0 : (d < 0.f ? 1.0 : 0.0)));
        } else {
            const double tt = t[i / per];
            const double lmc = -0.25 * (tt * tt) * (beta1 - beta0) - 0.5 * tt * beta0;   // vpsde.py:74-76
            const double sd = sqrt(1.0 - exp(2.0 * lmc));
            const double g2 = beta0 + tt * (beta1 - beta0);
            const double d = (-(double)ep[i] / sd) - (-(double)e[i] / sd);
            acc += d * d * g2;
            if (grad) grad[i] = (float)(gscale * 2.0 * d * g2 * (-1.0 / sd));
        }
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ void scaled_final_kernel(const double* __restrict__ part, int nparts, double denom, double* __restrict__ out64,
                                    float* __restrict__ out32) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) acc += part[i];
    acc = wave_sum_d(acc);
    if (threadIdx.x == 0) {
        if (out64) out64[0] = acc / denom;
        if (out32) out32[0] = (float)(acc / denom);
    }
}

extern "C" int psld_vp_score_loss(const float* eps, const float* eps_pred, const double* t, double beta0, double beta1,
                                  int batch, long long per, int mode, int reduce_mean, void* loss, float* grad,
                                  float grad_scale, void* workspace, hipStream_t stream) {
    PSLD_CHECK_ARG(eps && eps_pred && loss && workspace && batch > 0 && per > 0 && (mode == 1 || (mode == 2 && t)),
                   "psld_vp_score_loss: bad args");
    const long long n = (long long)batch * per;
    int blocks = grid_for(n);
    double* part = reinterpret_cast<double*>(workspace);
    const double denom = reduce_mean ? (double)n : 1.0;
    hipLaunchKernelGGL(vp_score_loss_kernel, dim3(blocks), dim3(256), 0, stream, eps, eps_pred, t, beta0, beta1, per, n,
                       mode, part, grad, (double)grad_scale / denom);
    PSLD_CHECK_LAUNCH("vp_score_loss_kernel");
    hipLaunchKernelGGL(scaled_final_kernel, dim3(1), dim3(64), 0, stream, part, blocks, denom,
                       mode == 2 ? reinterpret_cast<double*>(loss) : nullptr,
                       mode == 1 ? reinterpret_cast<float*>(loss) : nullptr);
    PSLD_CHECK_LAUNCH("scaled_final_kernel");
    return PSLD_OK;
}

// ---- likelihood-weighted PSLD score loss and its time sampler ---------------------------------------
// loss = sum_b sw_b sum_i g_x^2 e_x^2 + g_m^2 e_m^2 with e = score(eps_pred) - score(eps), score = -L_t^{-T} eps formed in
// f32 with the f32-cast coefficients exactly as get_score does (psld.py:230-260), g^2 of psld.py:375-377 and every product
// with it in f64.  One workgroup column per sample (blockIdx.y): the per-sample scalars are uniform over a workgroup, and
// the partial sums - one per workgroup, added up by scaled_final_kernel in index order - make the loss bitwise repeatable.
namespace {

struct NllCoeffs {
    float c11, c12, c21, c22;   // get_inv_coeff cast to f32 (psld.py:253-258)
    double gx2, gm2;            // beta(t) gamma, beta(t) M nu
};

__device__ NllCoeffs nll_coeffs(const psld_sde_params_t& p, const double* __restrict__ k, double tt) {
    const double xx = k[8], xm = k[9], mm = k[10];
    const double det = xx * mm - xm * xm;
    double c11, c12, c21, c22;
    if (p.decomp_lower) {  // psld.py:194-198
        c11 = sqrt(1.0 / xx);
        c12 = -xm / (sqrt(xx) * sqrt(det));
        c21 = 0.0;
        c22 = sqrt(xx / det);
    } else {  // psld.py:209-212
        c22 = sqrt(1.0 / mm);
        c21 = -xm / (sqrt(mm) * sqrt(det));
        c11 = sqrt(mm / det);
        c12 = 0.0;
    }
    const double beta = p.beta_0 + tt * (p.beta_1 - p.beta_0);
    NllCoeffs o;
    o.c11 = (float)c11; o.c12 = (float)c12; o.c21 = (float)c21; o.c22 = (float)c22;
    o.gx2 = beta * p.gamma;
    o.gm2 = beta * (1.0 / p.m_inv) * p.nu;
    return o;
}

// mode 0: one thread per VEC consecutive pixels of one channel plane of the x half and the same pixels of the m half
// (eps, eps_pred, grad [B,2C,HW]); modes 1 / 2: eps_pred and grad are [B,C,HW], the target is the m / x half of eps.
template <int VEC>
__global__ void nll_score_loss_kernel(const float* __restrict__ e, const float* __restrict__ ep,
                                      const double* __restrict__ t, const double* __restrict__ coeffs,
                                      const double* __restrict__ sw, const psld_sde_params_t p, int mode, long long plane,
                                      double gdenom, double* __restrict__ part, float* __restrict__ grad, float gscale) {
    typedef float fv __attribute__((ext_vector_type(VEC)));
    __shared__ double red[4];
    const int b = blockIdx.y;
    const NllCoeffs k = nll_coeffs(p, coeffs + (long long)b * COEFF_STRIDE, t[b]);
    const double w = sw ? sw[b] : 1.0;
    const double gs = 2.0 * w / gdenom;
    const long long items = plane / VEC;
    const long long e_base = (long long)b * 2 * items, p_base = (long long)b * (mode == 0 ? 2 : 1) * items;
    double acc = 0.0;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < items; r += (long long)gridDim.x * blockDim.x) {
        if (mode == 0) {
            const fv ex = reinterpret_cast<const fv*>(e)[e_base + r], em = reinterpret_cast<const fv*>(e)[e_base + items + r];
            const fv px = reinterpret_cast<const fv*>(ep)[p_base + r], pm = reinterpret_cast<const fv*>(ep)[p_base + items + r];
            fv gx, gm;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float dx = (-k.c11 * px[v] - k.c12 * pm[v]) - (-k.c11 * ex[v] - k.c12 * em[v]);
                const float dm = (-k.c21 * px[v] - k.c22 * pm[v]) - (-k.c21 * ex[v] - k.c22 * em[v]);
                const double ax = k.gx2 * (double)dx, am = k.gm2 * (double)dm;
                acc += ax * (double)dx + am * (double)dm;
                gx[v] = (float)(gs * (-(double)k.c11 * ax - (double)k.c21 * am)) * gscale;
                gm[v] = (float)(gs * (-(double)k.c12 * ax - (double)k.c22 * am)) * gscale;
            }
            if (grad) {
                reinterpret_cast<fv*>(grad)[p_base + r] = gx;
                reinterpret_cast<fv*>(grad)[p_base + items + r] = gm;
            }
        } else {
            const float c = mode == 1 ? k.c22 : k.c11;
            const double g2 = mode == 1 ? k.gm2 : k.gx2;
            const fv tv = reinterpret_cast<const fv*>(e)[e_base + (mode == 1 ? items : 0) + r];
            const fv pv = reinterpret_cast<const fv*>(ep)[p_base + r];
            fv gv;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                const float d = (-c * pv[v]) - (-c * tv[v]);
                const double a = g2 * (double)d;
                acc += a * (double)d;
                gv[v] = (float)(gs * (-(double)c * a)) * gscale;
            }
            if (grad) reinterpret_cast<fv*>(grad)[p_base + r] = gv;
        }
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long long)b * gridDim.x + blockIdx.x] = w * (red[0] + red[1] + red[2] + red[3]);
}

// t = the inverse CDF at u of the piecewise log-uniform density with bin masses ``mass`` on the edges exp(log_edges);
// weight = 1 / (q(t) span), q(t) = mass_k / (t (ln e_{k+1} - ln e_k))
__global__ void sample_times_kernel(const double* __restrict__ u, int batch, const double* __restrict__ cum,
                                    const double* __restrict__ log_edges, const double* __restrict__ mass, int bins,
                                    double span, double t_lo, double t_hi, double* __restrict__ t,
                                    double* __restrict__ weight) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch) return;
    const double uu = u[i];
    int lo = 0, hi = bins;   // the largest k < bins with cum[k] <= u (cum[0] = 0)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] <= uu) lo = mid; else hi = mid;
    }
    const double pk = mass[lo], dl = log_edges[lo + 1] - log_edges[lo];
    const double r = (uu - cum[lo]) / pk;
    double tt = exp(log_edges[lo] + r * dl);
    tt = tt < t_lo ? t_lo : (tt > t_hi ? t_hi : tt);
    t[i] = tt;
    weight[i] = tt * dl / (pk * span);
}

}  // namespace

extern "C" int psld_nll_score_loss(const float* eps, const float* eps_pred, const double* t, const double* coeffs,
                                   const double* sample_weight, const psld_sde_params_t* p, int score_mode, int batch,
                                   int c, int hw, int reduce_mean, double* loss, float* grad, float grad_scale,
                                   void* workspace, hipStream_t stream) {
    PSLD_CHECK_ARG(eps && eps_pred && t && coeffs && p && loss && workspace && batch > 0 && batch <= 4096 && c > 0 &&
                       hw > 0 && score_mode >= 0 && score_mode <= 2,
                   "psld_nll_score_loss: bad args (1 <= batch <= 4096, score_mode 0..2)");
    const long long plane = (long long)c * hw;
    const double n = 2.0 * (double)plane * batch;   // the element count of get_score's output in EVERY mode
    const double denom = reduce_mean ? n : 1.0;
    const bool vec = hw % 4 == 0 && ((reinterpret_cast<uintptr_t>(eps) | reinterpret_cast<uintptr_t>(eps_pred) |
                                      reinterpret_cast<uintptr_t>(grad)) & 15) == 0;
    const long long items = vec ? plane / 4 : plane;
    long long bx = (items + 255) / 256;
    const long long cap = 4096 / batch;   // batch * bx partial sums in a workspace of 4096
    if (bx > cap) bx = cap;
    double* part = reinterpret_cast<double*>(workspace);
    if (vec)
        hipLaunchKernelGGL(nll_score_loss_kernel<4>, dim3((unsigned)bx, batch), dim3(256), 0, stream, eps, eps_pred, t,
                           coeffs, sample_weight, *p, score_mode, plane, denom, part, grad, grad_scale);
    else
        hipLaunchKernelGGL(nll_score_loss_kernel<1>, dim3((unsigned)bx, batch), dim3(256), 0, stream, eps, eps_pred, t,
                           coeffs, sample_weight, *p, score_mode, plane, denom, part, grad, grad_scale);
    PSLD_CHECK_LAUNCH("nll_score_loss_kernel");
    hipLaunchKernelGGL(scaled_final_kernel, dim3(1), dim3(64), 0, stream, part, (int)(bx * batch), denom, loss, nullptr);
    PSLD_CHECK_LAUNCH("scaled_final_kernel");
    return PSLD_OK;
}

extern "C" int psld_sample_times_f64(const double* u, int batch, const double* cum, const double* log_edges,
                                     const double* mass, int bins, double span, double t_lo, double t_hi, double* t,
                                     double* weight, hipStream_t stream) {
    PSLD_CHECK_ARG(u && cum && log_edges && mass && t && weight && batch > 0 && bins > 0 && span > 0 && t_lo <= t_hi,
                   "psld_sample_times_f64: bad args");
    hipLaunchKernelGGL(sample_times_kernel, dim3(cdiv(batch, 128)), dim3(128), 0, stream, u, batch, cum, log_edges, mass,
                       bins, span, t_lo, t_hi, t, weight);
    PSLD_CHECK_LAUNCH("psld_sample_times_f64");
    return PSLD_OK;
}

// ---- probability-flow likelihood: probe, cotangent, augmented right-hand side, prior density ---------
// Streaming kernels around one vector-Jacobian product of the network per right-hand-side evaluation.  The two reductions
// (the divergence estimate, the Gaussian log-density) run as one workgroup per (sample, slice): the number of slices and
// every summation order follow from the SAMPLE's size alone, so a sample's value is bitwise the same in any batch.
namespace {

constexpr int PF_THREADS = 256;

// slices of a sample of ``items`` thread-items: one vector pass of a workgroup each, at most PSLD_PF_MAX_SLICES
inline int pf_slices(long long items) {
    const long long s = (items + 1023) / 1024;
    return (int)(s < 1 ? 1 : (s > PSLD_PF_MAX_SLICES ? PSLD_PF_MAX_SLICES : s));
}
inline bool pf_aligned(const void* q, uintptr_t a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; }

// +-1 from the dropout hash (common.h) at p = 1/2: element i is a function of (seed, offset + i) alone
template <int VEC>
__global__ void rademacher_kernel(float* __restrict__ out, long long n, unsigned long long seed,
                                  unsigned long long offset) {
    typedef float fv __attribute__((ext_vector_type(VEC)));
    const long long nv = n / VEC;
    GRID_STRIDE(i, nv) {
        fv v;
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            v[e] = psld_dropout_keep(seed, offset + (unsigned long long)(i * VEC + e), 0.5f) ? 1.f : -1.f;
        reinterpret_cast<fv*>(out)[i] = v;
    }
    if (VEC > 1 && blockIdx.x == 0 && (long long)threadIdx.x < n - nv * VEC) {
        const long long i = nv * VEC + threadIdx.x;
        out[i] = psld_dropout_keep(seed, offset + (unsigned long long)i, 0.5f) ? 1.f : -1.f;
    }
}

// w = A^T z with A: eps -> -1/2 g^2 s(eps), s = -L^{-T} eps (reverse_terms above); products in f64, rounded once
template <int VEC>
__global__ void pf_cotangent_kernel(const float* __restrict__ z, const psld_em_coeffs_t k, double vp_std, int c, int hw,
                                    float* __restrict__ w) {
    typedef float fv __attribute__((ext_vector_type(VEC)));
    const long long per = (long long)c * hw / VEC;
    const long long b = blockIdx.y;
    const fv* zv = reinterpret_cast<const fv*>(z);
    fv* wv = reinterpret_cast<fv*>(w);
    const double hx = 0.5 * k.beta * k.gamma, hm = 0.5 * k.beta * k.m * k.nu;
    const double axx = hx * (double)k.c11, axm = hm * (double)k.c21, amx = hx * (double)k.c12, amm = hm * (double)k.c22;
    const double avp = vp_std > 0.0 ? 0.5 * k.beta / vp_std : 0.0;
    for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < per; r += (long long)gridDim.x * blockDim.x) {
        if (vp_std > 0.0) {
            const fv zx = zv[b * per + r];
            fv o;
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = (float)(avp * (double)zx[e]);
            wv[b * per + r] = o;
        } else if (k.score_mode == 0) {
            const fv zx = zv[b * 2 * per + r], zm = zv[b * 2 * per + per + r];
            fv ox, om;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                ox[e] = (float)(axx * (double)zx[e] + axm * (double)zm[e]);
                om[e] = (float)(amx * (double)zx[e] + amm * (double)zm[e]);
            }
            wv[b * 2 * per + r] = ox;
            wv[b * 2 * per + per + r] = om;
        } else {
            const fv zz = zv[b * 2 * per + (k.score_mode == 1 ? per : 0) + r];
            const double a = k.score_mode == 1 ? amm : axx;
            fv o;
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = (float)(a * (double)zz[e]);
            wv[b * per + r] = o;
        }
    }
}

__device__ __forceinline__ void pf_block_sum(double acc, double* __restrict__ dst) {
    __shared__ double red[PF_THREADS / 64];
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) dst[0] = (red[0] + red[1]) + (red[2] + red[3]);
}

// forward-time drift F = f - 1/2 g^2 s = -f_bar(probability flow) of the kernels above, and this slice's share of z . vjp
template <int VEC>
__global__ void pf_div_rhs_kernel(const double* __restrict__ u, const float* __restrict__ eps, const float* __restrict__ vjp,
                                  const float* __restrict__ z, const psld_em_coeffs_t k, double vp_std, int c, int hw,
                                  double* __restrict__ out, double* __restrict__ part) {
    typedef float fv __attribute__((ext_vector_type(VEC)));
    typedef double dv __attribute__((ext_vector_type(VEC)));
    const long long per = (long long)c * hw / VEC;
    const long long b = blockIdx.y;
    const long long len = (per + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * len;
    const long long hi = lo + len < per ? lo + len : per;
    const dv* uv = reinterpret_cast<const dv*>(u);
    dv* fo = reinterpret_cast<dv*>(out);
    const fv* ev = reinterpret_cast<const fv*>(eps);
    const fv* jv = reinterpret_cast<const fv*>(vjp);
    const fv* zv = reinterpret_cast<const fv*>(z);
    double acc = 0.0;
    if (vp_std > 0.0) {
        const double g = sqrt(k.beta);
        for (long long r = lo + threadIdx.x; r < hi; r += blockDim.x) {
            const long long i = b * per + r;
            const dv xv = uv[i];
            const fv e4 = ev[i], j4 = jv[i], z4 = zv[i];
            dv f;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const double score = 0.5 * (-(double)e4[e] / vp_std);           // vp_reverse_kernel, probability flow
                f[e] = -(-(-0.5 * k.beta * xv[e]) + (g * g) * score);
                acc += (double)z4[e] * (double)j4[e];
            }
            fo[i] = f;
        }
    } else {
        for (long long r = lo + threadIdx.x; r < hi; r += blockDim.x) {
            const long long ox = b * 2 * per + r, om = ox + per;
            const dv xv = uv[ox], mv = uv[om];
            fv ex, em;
            if (k.score_mode == 0) { ex = ev[ox]; em = ev[om]; }
            else { ex = ev[b * per + r]; em = ex; }
            const fv jx = jv[ox], jm = jv[om], zx = zv[ox], zm = zv[om];
            dv fx, fm;
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const RevOut o = reverse_terms(k, xv[e], mv[e], ex[e], em[e], true);
                fx[e] = -o.fbx;
                fm[e] = -o.fbm;
                acc += (double)zx[e] * (double)jx[e];
            }
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc += (double)zm[e] * (double)jm[e];
            fo[ox] = fx;
            fo[om] = fm;
        }
    }
    pf_block_sum(acc, part + b * gridDim.x + blockIdx.x);
}

// one thread per sample: the slices' shares in slice order, on top of the analytic divergence of the linear drift
__global__ void pf_div_final_kernel(const double* __restrict__ part, int slices, int batch, double div_lin,
                                    double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double acc = 0.0;
    for (int s = 0; s < slices; ++s) acc += part[(long long)b * slices + s];
    out[b] = div_lin + acc;
}

// sums of squares of the first nx and of the other per - nx values of a sample, per slice
template <int VEC>
__global__ void gauss_sq_kernel(const double* __restrict__ u, long long nx, long long per, double* __restrict__ part) {
    typedef double dv __attribute__((ext_vector_type(VEC)));
    const long long items = per / VEC;
    const long long b = blockIdx.y;
    const long long len = (items + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * len;
    const long long hi = lo + len < items ? lo + len : items;
    const dv* uv = reinterpret_cast<const dv*>(u + b * per);
    double sx = 0.0, sm = 0.0;
    for (long long r = lo + threadIdx.x; r < hi; r += blockDim.x) {
        const dv v = uv[r];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            const double q = v[e] * v[e];
            if (r * VEC + e < nx) sx += q; else sm += q;
        }
    }
    double* dst = part + 2 * (b * gridDim.x + blockIdx.x);
    pf_block_sum(sx, dst);
    __syncthreads();
    pf_block_sum(sm, dst + 1);
}

__global__ void gauss_final_kernel(const double* __restrict__ part, int slices, int batch, double var_x, double var_m,
                                   long long nx, long long nm, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double sx = 0.0, sm = 0.0;
    for (int s = 0; s < slices; ++s) {
        sx += part[2 * ((long long)b * slices + s)];
        sm += part[2 * ((long long)b * slices + s) + 1];
    }
    const double two_pi = 6.283185307179586476925286766559;
    double lp = -0.5 * (sx / var_x) - 0.5 * ((double)nx * log(two_pi * var_x));
    if (nm > 0) lp = lp + (-0.5 * (sm / var_m) - 0.5 * ((double)nm * log(two_pi * var_m)));
    out[b] = lp;
}

}  // namespace

extern "C" long long psld_pf_workspace_bytes(int batch) {
    return 2LL * sizeof(double) * PSLD_PF_MAX_SLICES * (batch > 0 ? batch : 0);
}

extern "C" int psld_rademacher_f32(float* out, long long n, unsigned long long seed, unsigned long long offset,
                                   hipStream_t stream) {
    PSLD_CHECK_ARG(out && n > 0, "psld_rademacher_f32: bad args");
    if (pf_aligned(out, 16))
        hipLaunchKernelGGL(rademacher_kernel<4>, dim3(grid_for((n + 3) / 4)), dim3(256), 0, stream, out, n, seed, offset);
    else
        hipLaunchKernelGGL(rademacher_kernel<1>, dim3(grid_for(n)), dim3(256), 0, stream, out, n, seed, offset);
    PSLD_CHECK_LAUNCH("psld_rademacher_f32");
    return PSLD_OK;
}

extern "C" int psld_pf_cotangent_f32(const float* z, const psld_em_coeffs_t* k, double vp_std, int batch, int c, int hw,
                                     float* w, hipStream_t stream) {
    PSLD_CHECK_ARG(z && k && w && batch > 0 && batch <= 65535 && c > 0 && hw > 0 && vp_std >= 0.0 &&
                   (vp_std > 0.0 || (k->score_mode >= 0 && k->score_mode <= 2)), "psld_pf_cotangent_f32: bad args");
    const long long per = (long long)c * hw;
    if (hw % 4 == 0 && pf_aligned(z, 16) && pf_aligned(w, 16))
        hipLaunchKernelGGL(pf_cotangent_kernel<4>, dim3(pf_slices(per / 4), batch), dim3(PF_THREADS), 0, stream, z, *k, vp_std,
                           c, hw, w);
    else
        hipLaunchKernelGGL(pf_cotangent_kernel<1>, dim3(pf_slices(per), batch), dim3(PF_THREADS), 0, stream, z, *k, vp_std, c,
                           hw, w);
    PSLD_CHECK_LAUNCH("psld_pf_cotangent_f32");
    return PSLD_OK;
}

extern "C" int psld_pf_div_rhs_f64(const double* u, const float* eps_pred, const float* vjp, const float* z,
                                   const psld_em_coeffs_t* k, double vp_std, int batch, int c, int hw, double* out,
                                   void* workspace, hipStream_t stream) {
    PSLD_CHECK_ARG(u && eps_pred && vjp && z && k && out && workspace && batch > 0 && batch <= 65535 && c > 0 && hw > 0 &&
                   vp_std >= 0.0 && (vp_std > 0.0 || (k->score_mode >= 0 && k->score_mode <= 2)),
                   "psld_pf_div_rhs_f64: bad args");
    psld_em_coeffs_t kk = *k;
    kk.probability_flow = 1;
    const long long per = (long long)c * hw;
    const long long n = (vp_std > 0.0 ? 1 : 2) * per * batch;
    const double div_lin = (vp_std > 0.0 ? -0.5 * kk.beta : -0.5 * kk.beta * (kk.gamma + kk.nu)) * (double)per;
    double* part = reinterpret_cast<double*>(workspace);
    int slices;
    if (hw % 4 == 0 && pf_aligned(u, 32) && pf_aligned(out, 32) && pf_aligned(eps_pred, 16) && pf_aligned(vjp, 16) &&
        pf_aligned(z, 16)) {
        slices = pf_slices(per / 4);
        hipLaunchKernelGGL(pf_div_rhs_kernel<4>, dim3(slices, batch), dim3(PF_THREADS), 0, stream, u, eps_pred, vjp, z, kk,
                           vp_std, c, hw, out, part);
    } else {
        slices = pf_slices(per);
        hipLaunchKernelGGL(pf_div_rhs_kernel<1>, dim3(slices, batch), dim3(PF_THREADS), 0, stream, u, eps_pred, vjp, z, kk,
                           vp_std, c, hw, out, part);
    }
    PSLD_CHECK_LAUNCH("pf_div_rhs_kernel");
    hipLaunchKernelGGL(pf_div_final_kernel, dim3(cdiv(batch, 64)), dim3(64), 0, stream, part, slices, batch, div_lin, out + n);
    PSLD_CHECK_LAUNCH("pf_div_final_kernel");
    return PSLD_OK;
}

extern "C" int psld_gauss_logp_f64(const double* u, double var_x, double var_m, int batch, int c_x, int c_m, int hw,
                                   double* out, void* workspace, hipStream_t stream) {
    PSLD_CHECK_ARG(u && out && workspace && batch > 0 && batch <= 65535 && c_x > 0 && c_m >= 0 && hw > 0 && var_x > 0.0 &&
                   (c_m == 0 || var_m > 0.0), "psld_gauss_logp_f64: bad args");
    const long long nx = (long long)c_x * hw, nm = (long long)c_m * hw, per = nx + nm;
    double* part = reinterpret_cast<double*>(workspace);
    int slices;
    if (per % 2 == 0 && pf_aligned(u, 16)) {
        slices = pf_slices(per / 2);
        hipLaunchKernelGGL(gauss_sq_kernel<2>, dim3(slices, batch), dim3(PF_THREADS), 0, stream, u, nx, per, part);
    } else {
        slices = pf_slices(per);
        hipLaunchKernelGGL(gauss_sq_kernel<1>, dim3(slices, batch), dim3(PF_THREADS), 0, stream, u, nx, per, part);
    }
    PSLD_CHECK_LAUNCH("gauss_sq_kernel");
    hipLaunchKernelGGL(gauss_final_kernel, dim3(cdiv(batch, 64)), dim3(64), 0, stream, part, slices, batch, var_x, var_m, nx,
                       nm, out);
    PSLD_CHECK_LAUNCH("gauss_final_kernel");
    return PSLD_OK;
}
