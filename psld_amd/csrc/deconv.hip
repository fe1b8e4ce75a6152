// Measurement guidance for a blur, y = k (*) x0 + noise with a periodic boundary ("Deconvolution"; not in the reference):
// A A^T is no multiple of the identity, so the measure step needs (sigma_y^2 I + r_t^2 A A^T)^-1, which the 2-D DFT makes
// diagonal.  Three kernels around the per-plane transform of deconv_core.h, ONE workgroup per H x W plane at a time (a
// workgroup walks the planes blockIdx.x, blockIdx.x + gridDim.x, ...: any number of planes on any number of CUs):
//
//   measure:   x0^ = q_u . u - q_e . eps^ (as restore.hip), x^ = FFT2(x0^),
//              g^ = conj(h^) (sigma_y^2 + r_t^2) / (sigma_y^2 + r_t^2 |h^|^2) (y^ - h^ x^),  g = IFFT2(g^),  cotangent q_e g;
//   spectrum:  y^ = FFT2(y), the Hermitian half [H][W/2 + 1] in float64 - once per measurement;
//   apply:     A x = IFFT2(h^ x^) or A^T x = IFFT2(conj(h^) x^) - setting a problem up.
//
// And two more for super-resolution, A = D_s C_k: that blur followed by keeping the samples (s i, s j), s = 2 or 4 (DESIGN section
// 13, "Super-resolution").  A A^T is circulant on the H/s x W/s grid with eigenvalues Lambda (host float64), so the measure
// step is three transform pairs in the SAME plane storage - the low-resolution plane is compacted into the full one's place
// and expanded again (deconv_core.h, dc_sr_*) - and the apply kernel maps between the two resolutions:
//
//   sr measure: z = IFFT2(h^ FFT2 x0^), rho = y - D_s z, v = IFFT2'((sigma_y^2 + r_t^2) / (sigma_y^2 + r_t^2 Lambda) FFT2' rho),
//               g = IFFT2(conj(h^) FFT2(D_s^T v)), cotangent q_e g;
//   sr apply:   A x [H/s][W/s] = D_s IFFT2(h^ x^), or A^T r [H][W] = IFFT2(conj(h^) FFT2(D_s^T r)).
//
// float32 planes in memory; float64 in registers and LDS (towards sigma_y -> 0 the weight reaches 1 / |h^|, 1e4 and more for
// a Gaussian PSF: a float32 transform's rounding times that weight would leave the 1e-4 gate), float64 h^ and y^ in memory.
// LDS: H (W/2 + 1) + max(H, W) / 2 complex float64 - 131 KiB at 128 x 128, of a CU's 160 KiB; nothing beyond LDS.
// Compiled with -ffp-contract=off like restore.hip.
#include "common.h"
#include "deconv_core.h"
#include "psld_hip.h"

namespace {

constexpr int DC_THREADS = 256;
constexpr int DC_MIN = 4, DC_MAX = 128;

typedef float f4 __attribute__((ext_vector_type(4)));

// 4 consecutive floats: one 16-byte access (V16) or four 4-byte ones
template <bool V16>
__device__ __forceinline__ void dc_read4(const float* p, double (&v)[4]) {
    if constexpr (V16) {
        const f4 a = reinterpret_cast<const f4*>(p)[0];
        v[0] = (double)a[0]; v[1] = (double)a[1]; v[2] = (double)a[2]; v[3] = (double)a[3];
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (double)p[e];
    }
}
template <bool V16>
__device__ __forceinline__ void dc_write4(float* p, const double (&v)[4]) {
    if constexpr (V16) {
        f4 f;
        f[0] = (float)v[0]; f[1] = (float)v[1]; f[2] = (float)v[2]; f[3] = (float)v[3];
        reinterpret_cast<f4*>(p)[0] = f;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = (float)v[e];
    }
}

// plane element 4 i -> LDS element (row pitch p): W % 4 == 0, so 4 consecutive elements lie in one row
__device__ __forceinline__ int dc_lds_at(const dc_geom& g, int i4) {
    const int e = 4 * i4, r = e >> (g.lgm + 1), col = e & (2 * g.m - 1);
    return r * g.p + (col >> 1);
}

template <bool AUG, bool V16>
__global__ __launch_bounds__(DC_THREADS) void restore_deconv_kernel(const float* __restrict__ u, const float* __restrict__ eps,
                                                                     const dc2* __restrict__ yhat, const dc2* __restrict__ hhat,
                                                                     const psld_restore_coeffs_t q, double s2, double r2,
                                                                     int planes, int c, dc_geom g, float* __restrict__ gout,
                                                                     float* __restrict__ cot) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dc_lds_raw[];
    dc2* z = reinterpret_cast<dc2*>(dc_lds_raw);
    dc2* tw = z + dc_plane_elems(g);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long long hw = (long long)g.h * 2 * g.m, spec = (long long)g.h * (g.m + 1);
    const double inv = 1.0 / (double)(g.h * g.m);
    dc_twiddles(tw, g, tid, nthr);
    for (int pl = blockIdx.x; pl < planes; pl += gridDim.x) {
        const int b = pl / c, ch = pl - b * c;
        const long long ox = ((long long)(AUG ? b * 2 * c + ch : pl)) * hw, om = ox + (long long)c * hw, og = (long long)pl * hw;
        DC_FOR(i, (int)(hw / 4)) {
            double ux[4], ex[4], x0[4];
            dc_read4<V16>(u + ox + 4 * i, ux);
            dc_read4<V16>(eps + ox + 4 * i, ex);
            if constexpr (AUG) {
                double um[4], em[4];
                dc_read4<V16>(u + om + 4 * i, um);
                dc_read4<V16>(eps + om + 4 * i, em);
#pragma unroll
                for (int e = 0; e < 4; ++e) x0[e] = ((q.q_u[0] * ux[e] + q.q_u[1] * um[e]) - q.q_e[0] * ex[e]) - q.q_e[1] * em[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x0[e] = q.q_u[0] * ux[e] - q.q_e[0] * ex[e];
            }
            const int at = dc_lds_at(g, i);
            z[at] = dc_make(x0[0], x0[1]);
            z[at + 1] = dc_make(x0[2], x0[3]);
        }
        __syncthreads();
        dc_forward(z, tw, g, tid, nthr);
        dc_measure_filter f{hhat, yhat + (long long)pl * spec, s2, r2};
        dc_filter<false>(z, tw, g, f, nullptr, tid, nthr);
        dc_inverse(z, tw, g, tid, nthr);
        DC_FOR(i, (int)(hw / 4)) {
            const int at = dc_lds_at(g, i);
            const dc2 a = z[at], d = z[at + 1];
            const double gv[4] = {a.x * inv, a.y * inv, d.x * inv, d.y * inv};
            double w[4];
            dc_write4<V16>(gout + og + 4 * i, gv);
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = q.q_e[0] * gv[e];
            dc_write4<V16>(cot + ox + 4 * i, w);
            if constexpr (AUG) {
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = q.q_e[1] * gv[e];
                dc_write4<V16>(cot + om + 4 * i, w);
            }
        }
        __syncthreads();  // the next plane overwrites z
    }
}

// MODE 0: out = A x, 1: out = A^T x (float32 planes), 2: spec = FFT2(x) (the Hermitian half, float64)
template <int MODE, bool V16>
__global__ __launch_bounds__(DC_THREADS) void restore_deconv_plane_kernel(const float* __restrict__ x, const dc2* __restrict__ hhat,
                                                                           int planes, dc_geom g, float* __restrict__ out,
                                                                           dc2* __restrict__ spec_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dc_lds_raw[];
    dc2* z = reinterpret_cast<dc2*>(dc_lds_raw);
    dc2* tw = z + dc_plane_elems(g);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const long long hw = (long long)g.h * 2 * g.m, spec = (long long)g.h * (g.m + 1);
    const double inv = 1.0 / (double)(g.h * g.m);
    dc_twiddles(tw, g, tid, nthr);
    for (int pl = blockIdx.x; pl < planes; pl += gridDim.x) {
        DC_FOR(i, (int)(hw / 4)) {
            double v[4];
            dc_read4<V16>(x + (long long)pl * hw + 4 * i, v);
            const int at = dc_lds_at(g, i);
            z[at] = dc_make(v[0], v[1]);
            z[at + 1] = dc_make(v[2], v[3]);
        }
        __syncthreads();
        dc_forward(z, tw, g, tid, nthr);
        dc_apply_filter f{hhat, MODE == 1};
        if constexpr (MODE == 2) {
            dc_filter<true>(z, tw, g, f, spec_out + (long long)pl * spec, tid, nthr);
        } else {
            dc_filter<false>(z, tw, g, f, nullptr, tid, nthr);
            dc_inverse(z, tw, g, tid, nthr);
            DC_FOR(i, (int)(hw / 4)) {
                const int at = dc_lds_at(g, i);
                const dc2 a = z[at], d = z[at + 1];
                const double v[4] = {a.x * inv, a.y * inv, d.x * inv, d.y * inv};
                dc_write4<V16>(out + (long long)pl * hw + 4 * i, v);
            }
            __syncthreads();
        }
    }
}

// ---- super-resolution ("Super-resolution"): A = D_s C_k, y at H/s x W/s ---------------------------------------
// 4 low-resolution samples (i, col .. col + 3) of one float32 plane with rows of wl elements
template <bool V16>
struct sr_load4 {
    const float* p;
    int wl;
    __device__ __forceinline__ void operator()(int i, int col, double (&v)[4]) const { dc_read4<V16>(p + (long long)i * wl + col, v); }
};
template <bool V16>
struct sr_store4 {
    float* p;
    int wl;
    __device__ __forceinline__ void operator()(int i, int col, const double (&v)[4]) const { dc_write4<V16>(p + (long long)i * wl + col, v); }
};

// the measure step: three transform pairs on the one plane storage (deconv_core.h)
template <bool AUG, bool V16>
__global__ __launch_bounds__(DC_THREADS) void restore_sr_kernel(const float* __restrict__ u, const float* __restrict__ eps,
                                                                 const float* __restrict__ y, const dc2* __restrict__ hhat,
                                                                 const double* __restrict__ lam, const psld_restore_coeffs_t q,
                                                                 double s2, double r2, int planes, int c, dc_geom g, int s, int lgs,
                                                                 float* __restrict__ gout, float* __restrict__ cot) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dc_lds_raw[];
    dc2* z = reinterpret_cast<dc2*>(dc_lds_raw);
    dc2* tw = z + dc_plane_elems(g);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const dc_geom gl = dc_sr_low(g, s, lgs);
    const long long hw = (long long)g.h * 2 * g.m, hwl = (long long)gl.h * 2 * gl.m;
    const double inv = 1.0 / (double)(g.h * g.m), invl = 1.0 / (double)(gl.h * gl.m);
    dc_twiddles(tw, g, tid, nthr);
    for (int pl = blockIdx.x; pl < planes; pl += gridDim.x) {
        const int b = pl / c, ch = pl - b * c;
        const long long ox = ((long long)(AUG ? b * 2 * c + ch : pl)) * hw, om = ox + (long long)c * hw, og = (long long)pl * hw;
        DC_FOR(i, (int)(hw / 4)) {
            double ux[4], ex[4], x0[4];
            dc_read4<V16>(u + ox + 4 * i, ux);
            dc_read4<V16>(eps + ox + 4 * i, ex);
            if constexpr (AUG) {
                double um[4], em[4];
                dc_read4<V16>(u + om + 4 * i, um);
                dc_read4<V16>(eps + om + 4 * i, em);
#pragma unroll
                for (int e = 0; e < 4; ++e) x0[e] = ((q.q_u[0] * ux[e] + q.q_u[1] * um[e]) - q.q_e[0] * ex[e]) - q.q_e[1] * em[e];
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) x0[e] = q.q_u[0] * ux[e] - q.q_e[0] * ex[e];
            }
            const int at = dc_lds_at(g, i);
            z[at] = dc_make(x0[0], x0[1]);
            z[at + 1] = dc_make(x0[2], x0[3]);
        }
        __syncthreads();
        // z = k (*) x0^
        dc_forward(z, tw, g, tid, nthr);
        dc_filter<false>(z, tw, g, dc_apply_filter{hhat, false}, nullptr, tid, nthr);
        dc_inverse(z, tw, g, tid, nthr);
        // rho = y - D_s z, then v = (s2 + r2) (s2 I + r2 A A^T)^-1 rho on the low-resolution grid
        dc_sr_residual(z, g, gl, s, inv, sr_load4<V16>{y + (long long)pl * hwl, 2 * gl.m}, tid, nthr);
        dc_forward(z, tw, gl, tid, nthr);
        dc_filter<false>(z, tw, gl, dc_sr_solve_filter{lam, s2, r2}, nullptr, tid, nthr);
        dc_inverse(z, tw, gl, tid, nthr);
        // g = A^T v = conj(k) (*) D_s^T v
        dc_sr_zero_insert(z, g, gl, s, invl, tid, nthr);
        dc_forward(z, tw, g, tid, nthr);
        dc_filter<false>(z, tw, g, dc_apply_filter{hhat, true}, nullptr, tid, nthr);
        dc_inverse(z, tw, g, tid, nthr);
        DC_FOR(i, (int)(hw / 4)) {
            const int at = dc_lds_at(g, i);
            const dc2 a = z[at], d = z[at + 1];
            const double gv[4] = {a.x * inv, a.y * inv, d.x * inv, d.y * inv};
            double w[4];
            dc_write4<V16>(gout + og + 4 * i, gv);
#pragma unroll
            for (int e = 0; e < 4; ++e) w[e] = q.q_e[0] * gv[e];
            dc_write4<V16>(cot + ox + 4 * i, w);
            if constexpr (AUG) {
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = q.q_e[1] * gv[e];
                dc_write4<V16>(cot + om + 4 * i, w);
            }
        }
        __syncthreads();  // the next plane overwrites z
    }
}

// ADJ false: out [planes][h/s][w/s] = A x of x [planes][h][w]; true: out [planes][h][w] = A^T x of x [planes][h/s][w/s]
template <bool ADJ, bool V16>
__global__ __launch_bounds__(DC_THREADS) void restore_sr_apply_kernel(const float* __restrict__ x, const dc2* __restrict__ hhat,
                                                                       int planes, dc_geom g, int s, int lgs, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dc_lds_raw[];
    dc2* z = reinterpret_cast<dc2*>(dc_lds_raw);
    dc2* tw = z + dc_plane_elems(g);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const dc_geom gl = dc_sr_low(g, s, lgs);
    const long long hw = (long long)g.h * 2 * g.m, hwl = (long long)gl.h * 2 * gl.m;
    const double inv = 1.0 / (double)(g.h * g.m);
    dc_twiddles(tw, g, tid, nthr);
    for (int pl = blockIdx.x; pl < planes; pl += gridDim.x) {
        if constexpr (ADJ) {
            dc_sr_spread(z, g, gl, s, sr_load4<V16>{x + (long long)pl * hwl, 2 * gl.m}, tid, nthr);
        } else {
            DC_FOR(i, (int)(hw / 4)) {
                double v[4];
                dc_read4<V16>(x + (long long)pl * hw + 4 * i, v);
                const int at = dc_lds_at(g, i);
                z[at] = dc_make(v[0], v[1]);
                z[at + 1] = dc_make(v[2], v[3]);
            }
            __syncthreads();
        }
        dc_forward(z, tw, g, tid, nthr);
        dc_filter<false>(z, tw, g, dc_apply_filter{hhat, ADJ}, nullptr, tid, nthr);
        dc_inverse(z, tw, g, tid, nthr);
        if constexpr (ADJ) {
            DC_FOR(i, (int)(hw / 4)) {
                const int at = dc_lds_at(g, i);
                const dc2 a = z[at], d = z[at + 1];
                const double v[4] = {a.x * inv, a.y * inv, d.x * inv, d.y * inv};
                dc_write4<V16>(out + (long long)pl * hw + 4 * i, v);
            }
            __syncthreads();
        } else {
            dc_sr_decimate(z, g, gl, s, inv, sr_store4<V16>{out + (long long)pl * hwl, 2 * gl.m}, tid, nthr);
        }
    }
}

inline int dc_log2(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}
inline bool dc_size_ok(int n) { return n >= DC_MIN && n <= DC_MAX && (n & (n - 1)) == 0; }

// workgroups of a launch: one per plane, at most 4 waves of them over the 256 CUs
inline int dc_grid(long long planes) { return (int)(planes < 1024 ? planes : 1024); }

template <auto Kernel, class... Args>
int dc_launch(const char* name, long long planes, const dc_geom& g, hipStream_t stream, Args... args) {
    const size_t lds = (size_t)dc_lds_elems(g) * sizeof(dc2);
    // one limit for every shape: the largest plane's
    const dc_geom big = dc_geometry(DC_MAX, DC_MAX, 7, 7);
    if (int rc = psld_lds_once<Kernel>((size_t)dc_lds_elems(big) * sizeof(dc2), name)) return rc;
    hipLaunchKernelGGL(Kernel, dim3(dc_grid(planes)), dim3(DC_THREADS), lds, stream, args...);
    return PSLD_OK;
}

}  // namespace

extern "C" int psld_restore_deconv_supported(int h, int w) { return dc_size_ok(h) && dc_size_ok(w) ? 1 : 0; }

extern "C" int psld_restore_deconv_f32(const float* u, const float* eps, const double* yhat, const double* hhat,
                                       const psld_restore_coeffs_t* q, double sigma_y2, double r2, int batch, int c, int h,
                                       int w, float* g, float* cot, hipStream_t stream) {
    PSLD_CHECK_ARG(u && eps && yhat && hhat && q && g && cot && batch > 0 && c > 0, "psld_restore_deconv_f32: bad args");
    PSLD_CHECK_ARG(psld_restore_deconv_supported(h, w),
                   "psld_restore_deconv_f32: map %d x %d: each side must be a power of two from %d to %d", h, w, DC_MIN, DC_MAX);
    PSLD_CHECK_ARG(q->augmented == 0 || q->augmented == 1, "psld_restore_deconv_f32: augmented %d not 0 / 1", q->augmented);
    PSLD_CHECK_ARG(sigma_y2 >= 0.0 && r2 >= 0.0 && sigma_y2 + r2 > 0.0 && sigma_y2 + r2 < HUGE_VAL,
                   "psld_restore_deconv_f32: sigma_y^2 = %g, r_t^2 = %g: both must be >= 0 with a positive finite sum", sigma_y2, r2);
    PSLD_CHECK_ARG((long long)batch * c <= 0x7fffffffLL / 2, "psld_restore_deconv_f32: %lld planes are too many", (long long)batch * c);
    PSLD_CHECK_ARG(((uintptr_t)yhat | (uintptr_t)hhat) % 16 == 0, "psld_restore_deconv_f32: yhat and hhat must be 16-byte aligned");
    const dc_geom geo = dc_geometry(h, w, dc_log2(h), dc_log2(w));
    const int planes = batch * c;
    const bool v16 = ((uintptr_t)u | (uintptr_t)eps | (uintptr_t)g | (uintptr_t)cot) % 16 == 0;
    const dc2* yh = reinterpret_cast<const dc2*>(yhat);
    const dc2* hh = reinterpret_cast<const dc2*>(hhat);
    const char* name = "psld_restore_deconv_f32";
    int rc;
    if (q->augmented) {
        rc = v16 ? dc_launch<&restore_deconv_kernel<true, true>>(name, planes, geo, stream, u, eps, yh, hh, *q, sigma_y2, r2, planes, c, geo, g, cot)
                 : dc_launch<&restore_deconv_kernel<true, false>>(name, planes, geo, stream, u, eps, yh, hh, *q, sigma_y2, r2, planes, c, geo, g, cot);
    } else {
        rc = v16 ? dc_launch<&restore_deconv_kernel<false, true>>(name, planes, geo, stream, u, eps, yh, hh, *q, sigma_y2, r2, planes, c, geo, g, cot)
                 : dc_launch<&restore_deconv_kernel<false, false>>(name, planes, geo, stream, u, eps, yh, hh, *q, sigma_y2, r2, planes, c, geo, g, cot);
    }
    if (rc) return rc;
    PSLD_CHECK_LAUNCH(name);
    return PSLD_OK;
}

extern "C" int psld_restore_deconv_spectrum_f32(const float* y, int planes, int h, int w, double* yhat, hipStream_t stream) {
    PSLD_CHECK_ARG(y && yhat && planes > 0 && planes <= 0x7fffffff / 2, "psld_restore_deconv_spectrum_f32: bad args");
    PSLD_CHECK_ARG(psld_restore_deconv_supported(h, w),
                   "psld_restore_deconv_spectrum_f32: map %d x %d: each side must be a power of two from %d to %d", h, w, DC_MIN, DC_MAX);
    PSLD_CHECK_ARG((uintptr_t)yhat % 16 == 0, "psld_restore_deconv_spectrum_f32: yhat must be 16-byte aligned");
    const dc_geom geo = dc_geometry(h, w, dc_log2(h), dc_log2(w));
    const char* name = "psld_restore_deconv_spectrum_f32";
    dc2* yh = reinterpret_cast<dc2*>(yhat);
    const int rc = (uintptr_t)y % 16 == 0
                       ? dc_launch<&restore_deconv_plane_kernel<2, true>>(name, planes, geo, stream, y, (const dc2*)nullptr, planes, geo, (float*)nullptr, yh)
                       : dc_launch<&restore_deconv_plane_kernel<2, false>>(name, planes, geo, stream, y, (const dc2*)nullptr, planes, geo, (float*)nullptr, yh);
    if (rc) return rc;
    PSLD_CHECK_LAUNCH(name);
    return PSLD_OK;
}

extern "C" int psld_restore_deconv_apply_f32(const float* x, const double* hhat, int adjoint, int planes, int h, int w,
                                             float* out, hipStream_t stream) {
    PSLD_CHECK_ARG(x && hhat && out && planes > 0 && planes <= 0x7fffffff / 2, "psld_restore_deconv_apply_f32: bad args");
    PSLD_CHECK_ARG(adjoint == 0 || adjoint == 1, "psld_restore_deconv_apply_f32: adjoint %d not 0 / 1", adjoint);
    PSLD_CHECK_ARG(psld_restore_deconv_supported(h, w),
                   "psld_restore_deconv_apply_f32: map %d x %d: each side must be a power of two from %d to %d", h, w, DC_MIN, DC_MAX);
    PSLD_CHECK_ARG((uintptr_t)hhat % 16 == 0, "psld_restore_deconv_apply_f32: hhat must be 16-byte aligned");
    const dc_geom geo = dc_geometry(h, w, dc_log2(h), dc_log2(w));
    const char* name = "psld_restore_deconv_apply_f32";
    const dc2* hh = reinterpret_cast<const dc2*>(hhat);
    const bool v16 = ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
    int rc;
    if (adjoint)
        rc = v16 ? dc_launch<&restore_deconv_plane_kernel<1, true>>(name, planes, geo, stream, x, hh, planes, geo, out, (dc2*)nullptr)
                 : dc_launch<&restore_deconv_plane_kernel<1, false>>(name, planes, geo, stream, x, hh, planes, geo, out, (dc2*)nullptr);
    else
        rc = v16 ? dc_launch<&restore_deconv_plane_kernel<0, true>>(name, planes, geo, stream, x, hh, planes, geo, out, (dc2*)nullptr)
                 : dc_launch<&restore_deconv_plane_kernel<0, false>>(name, planes, geo, stream, x, hh, planes, geo, out, (dc2*)nullptr);
    if (rc) return rc;
    PSLD_CHECK_LAUNCH(name);
    return PSLD_OK;
}

extern "C" int psld_restore_sr_supported(int h, int w, int s) {
    return (s == 2 || s == 4) && dc_size_ok(h) && dc_size_ok(w) && h / s >= DC_MIN && w / s >= DC_MIN ? 1 : 0;
}

extern "C" int psld_restore_sr_f32(const float* u, const float* eps, const float* y, const double* hhat, const double* lam,
                                   const psld_restore_coeffs_t* q, double sigma_y2, double r2, int batch, int c, int h, int w,
                                   int s, float* g, float* cot, hipStream_t stream) {
    PSLD_CHECK_ARG(u && eps && y && hhat && lam && q && g && cot && batch > 0 && c > 0, "psld_restore_sr_f32: bad args");
    PSLD_CHECK_ARG(psld_restore_sr_supported(h, w, s),
                   "psld_restore_sr_f32: map %d x %d, factor %d: the factor must be 2 or 4 and each side a power of two from %d to %d",
                   h, w, s, DC_MIN * (s > 0 ? s : 1), DC_MAX);
    PSLD_CHECK_ARG(q->augmented == 0 || q->augmented == 1, "psld_restore_sr_f32: augmented %d not 0 / 1", q->augmented);
    PSLD_CHECK_ARG(sigma_y2 >= 0.0 && r2 >= 0.0 && sigma_y2 + r2 > 0.0 && sigma_y2 + r2 < HUGE_VAL,
                   "psld_restore_sr_f32: sigma_y^2 = %g, r_t^2 = %g: both must be >= 0 with a positive finite sum", sigma_y2, r2);
    PSLD_CHECK_ARG((long long)batch * c <= 0x7fffffffLL / 2, "psld_restore_sr_f32: %lld planes are too many", (long long)batch * c);
    PSLD_CHECK_ARG((uintptr_t)hhat % 16 == 0 && (uintptr_t)lam % 8 == 0,
                   "psld_restore_sr_f32: hhat must be 16-byte aligned and lam 8-byte aligned");
    const dc_geom geo = dc_geometry(h, w, dc_log2(h), dc_log2(w));
    const int planes = batch * c, lgs = dc_log2(s);
    const bool v16 = ((uintptr_t)u | (uintptr_t)eps | (uintptr_t)y | (uintptr_t)g | (uintptr_t)cot) % 16 == 0;
    const dc2* hh = reinterpret_cast<const dc2*>(hhat);
    const char* name = "psld_restore_sr_f32";
    int rc;
    if (q->augmented) {
        rc = v16 ? dc_launch<&restore_sr_kernel<true, true>>(name, planes, geo, stream, u, eps, y, hh, lam, *q, sigma_y2, r2, planes, c, geo, s, lgs, g, cot)
                 : dc_launch<&restore_sr_kernel<true, false>>(name, planes, geo, stream, u, eps, y, hh, lam, *q, sigma_y2, r2, planes, c, geo, s, lgs, g, cot);
    } else {
        rc = v16 ? dc_launch<&restore_sr_kernel<false, true>>(name, planes, geo, stream, u, eps, y, hh, lam, *q, sigma_y2, r2, planes, c, geo, s, lgs, g, cot)
                 : dc_launch<&restore_sr_kernel<false, false>>(name, planes, geo, stream, u, eps, y, hh, lam, *q, sigma_y2, r2, planes, c, geo, s, lgs, g, cot);
    }
    if (rc) return rc;
    PSLD_CHECK_LAUNCH(name);
    return PSLD_OK;
}

extern "C" int psld_restore_sr_apply_f32(const float* x, const double* hhat, int adjoint, int planes, int h, int w, int s,
                                         float* out, hipStream_t stream) {
    PSLD_CHECK_ARG(x && hhat && out && planes > 0 && planes <= 0x7fffffff / 2, "psld_restore_sr_apply_f32: bad args");
    PSLD_CHECK_ARG(adjoint == 0 || adjoint == 1, "psld_restore_sr_apply_f32: adjoint %d not 0 / 1", adjoint);
    PSLD_CHECK_ARG(psld_restore_sr_supported(h, w, s),
                   "psld_restore_sr_apply_f32: map %d x %d, factor %d: the factor must be 2 or 4 and each side a power of two from %d to %d",
                   h, w, s, DC_MIN * (s > 0 ? s : 1), DC_MAX);
    PSLD_CHECK_ARG((uintptr_t)hhat % 16 == 0, "psld_restore_sr_apply_f32: hhat must be 16-byte aligned");
    const dc_geom geo = dc_geometry(h, w, dc_log2(h), dc_log2(w));
    const int lgs = dc_log2(s);
    const char* name = "psld_restore_sr_apply_f32";
    const dc2* hh = reinterpret_cast<const dc2*>(hhat);
    const bool v16 = ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
    int rc;
    if (adjoint)
        rc = v16 ? dc_launch<&restore_sr_apply_kernel<true, true>>(name, planes, geo, stream, x, hh, planes, geo, s, lgs, out)
                 : dc_launch<&restore_sr_apply_kernel<true, false>>(name, planes, geo, stream, x, hh, planes, geo, s, lgs, out);
    else
        rc = v16 ? dc_launch<&restore_sr_apply_kernel<false, true>>(name, planes, geo, stream, x, hh, planes, geo, s, lgs, out)
                 : dc_launch<&restore_sr_apply_kernel<false, false>>(name, planes, geo, stream, x, hh, planes, geo, s, lgs, out);
    if (rc) return rc;
    PSLD_CHECK_LAUNCH(name);
    return PSLD_OK;
}
