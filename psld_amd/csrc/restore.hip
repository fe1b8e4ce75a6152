// Measurement-guided (posterior) sampling for linear inverse problems y = A x0 + noise (not in the
// reference): the two streaming kernels around the ONE network evaluation with its input gradient that a guided call costs.
//
//   measure:  x0^ = q_u . u - q_e . eps^   (the Tweedie estimate of the clean image from the state and the network output)
//             r = y - A x0^,  g = A^T r,   cotangent w = q_e g  (what the input-gradient-only backward is fed)
//   combine:  eps^' = eps^ - kappa (q_e g - L^T dx),  dx = J^T w
//
// float32 tensors, float64 arithmetic in registers (x0^ cancels three digits towards t -> T), coefficients from the host in
// float64.  Compiled with -ffp-contract=off like sde.hip: the operation order written here is the one the float64
// restatement of the tests follows.  A thread handles what its operator couples: one element (mask), the three channels of
// a pixel (gray), one k x k block of one channel (pool).  All public tensors are NCHW.
#include "common.h"
#include "psld_hip.h"

namespace {

#define GRID_STRIDE(i, n) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

inline int grid_for(long long n) {
    long long b = (n + 255) / 256;
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    return (int)b;
}

typedef float f4 __attribute__((ext_vector_type(4)));

// V16: one 16-byte access (VEC == 4 only); else element by element
template <int VEC, bool V16 = (VEC == 4)>
__device__ __forceinline__ void rs_read(const float* p, float (&v)[VEC]) {
    if constexpr (V16) {
        static_assert(VEC == 4, "16-byte accesses move 4 floats");
        const f4 a = reinterpret_cast<const f4*>(p)[0];
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) v[e] = p[e];
    }
}
// the float32 rounding of float64 values
template <int VEC, bool V16 = (VEC == 4)>
__device__ __forceinline__ void rs_write(float* p, const double (&v)[VEC]) {
    if constexpr (V16) {
        f4 f;
        f[0] = (float)v[0]; f[1] = (float)v[1]; f[2] = (float)v[2]; f[3] = (float)v[3];
        reinterpret_cast<f4*>(p)[0] = f;
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) p[e] = (float)v[e];
    }
}

// x0^ of VEC elements: state and eps at element offset ox (and om = the momentum half, augmented only)
template <int VEC, bool AUG, bool V16 = (VEC == 4)>
__device__ __forceinline__ void rs_x0(const float* __restrict__ u, const float* __restrict__ eps,
                                      const psld_restore_coeffs_t& q, long long ox, long long om, double (&x0)[VEC]) {
    float ux[VEC], ex[VEC];
    rs_read<VEC, V16>(u + ox, ux);
    rs_read<VEC, V16>(eps + ox, ex);
    if constexpr (AUG) {
        float um[VEC], em[VEC];
        rs_read<VEC, V16>(u + om, um);
        rs_read<VEC, V16>(eps + om, em);
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            x0[e] = ((q.q_u[0] * (double)ux[e] + q.q_u[1] * (double)um[e]) - q.q_e[0] * (double)ex[e]) - q.q_e[1] * (double)em[e];
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e) x0[e] = q.q_u[0] * (double)ux[e] - q.q_e[0] * (double)ex[e];
    }
}

// g and the cotangent q_e g (of the unrounded g) of VEC elements: g at og, the cotangent at ox / om like the state
template <int VEC, bool AUG, bool V16 = (VEC == 4)>
__device__ __forceinline__ void rs_put(float* __restrict__ g, float* __restrict__ cot, const psld_restore_coeffs_t& q,
                                       long long og, long long ox, long long om, const double (&gv)[VEC]) {
    double w[VEC];
    rs_write<VEC, V16>(g + og, gv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) w[e] = q.q_e[0] * gv[e];
    rs_write<VEC, V16>(cot + ox, w);
    if constexpr (AUG) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) w[e] = q.q_e[1] * gv[e];
        rs_write<VEC, V16>(cot + om, w);
    }
}

// ---- mask: A x = M . x ------------------------------------------------------------------------------------------------
template <int VEC, bool AUG>
__device__ __forceinline__ void measure_mask_at(const float* __restrict__ u, const float* __restrict__ eps,
                                                const float* __restrict__ y, const float* __restrict__ mask,
                                                const psld_restore_coeffs_t& q, long long og, long long ox, long long om,
                                                float* __restrict__ g, float* __restrict__ cot) {
    double x0[VEC], gv[VEC];
    float yv[VEC], mv[VEC];
    rs_x0<VEC, AUG>(u, eps, q, ox, om, x0);
    rs_read<VEC>(y + og, yv);
    rs_read<VEC>(mask + og, mv);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const double m = (double)mv[e];
        gv[e] = m * ((double)yv[e] - m * x0[e]);
    }
    rs_put<VEC, AUG>(g, cot, q, og, ox, om, gv);
}

// nseg segments of `seg` elements (sde.hip's ei_step_kernel): segment s of the state starts at element s * stride, segment
// s of g, y and the mask at s * seg.  The first seg / VEC * VEC elements of a segment go VEC at a time, the rest one at a
// time (only the flat state, which is ONE segment of any length).
template <int VEC, bool AUG>
__global__ void restore_measure_mask_kernel(const float* __restrict__ u, const float* __restrict__ eps,
                                            const float* __restrict__ y, const float* __restrict__ mask,
                                            const psld_restore_coeffs_t q, long long nseg, long long seg, long long stride,
                                            float* __restrict__ g, float* __restrict__ cot) {
    const long long pv = seg / VEC, nvec = nseg * pv;
    GRID_STRIDE(i, nvec) {
        const long long s = i / pv, r = (i - s * pv) * VEC;
        const long long ox = s * stride + r;
        measure_mask_at<VEC, AUG>(u, eps, y, mask, q, s * seg + r, ox, ox + seg, g, cot);
    }
    if constexpr (VEC > 1) {
        const long long tail = seg - pv * VEC, ntail = nseg * tail;
        GRID_STRIDE(i, ntail) {
            const long long s = i / tail, r = pv * VEC + (i - s * tail);
            const long long ox = s * stride + r;
            measure_mask_at<1, AUG>(u, eps, y, mask, q, s * seg + r, ox, ox + seg, g, cot);
        }
    }
}

// ---- gray: A x = (x_R + x_G + x_B) / sqrt(3); VEC pixels (hw % VEC == 0) and their three channels per thread ------------
template <int VEC, bool AUG>
__global__ void restore_measure_gray_kernel(const float* __restrict__ u, const float* __restrict__ eps,
                                            const float* __restrict__ y, const psld_restore_coeffs_t q, double a,
                                            long long batch, long long hw, float* __restrict__ g, float* __restrict__ cot) {
    const long long pv = hw / VEC, nvec = batch * pv;
    const long long ct = AUG ? 6 : 3;
    GRID_STRIDE(i, nvec) {
        const long long b = i / pv, p = (i - b * pv) * VEC;
        double x0[3][VEC], gv[VEC];
        float yv[VEC];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const long long ox = (b * ct + ch) * hw + p;
            rs_x0<VEC, AUG>(u, eps, q, ox, ox + 3 * hw, x0[ch]);
        }
        rs_read<VEC>(y + b * hw + p, yv);
#pragma unroll
        for (int e = 0; e < VEC; ++e) gv[e] = a * ((double)yv[e] - a * ((x0[0][e] + x0[1][e]) + x0[2][e]));
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const long long ox = (b * ct + ch) * hw + p;
            rs_put<VEC, AUG>(g, cot, q, (b * 3 + ch) * hw + p, ox, ox + 3 * hw, gv);
        }
    }
}

// ---- pool: A x = (1 / K) sum over each K x K block; NB blocks side by side (a strip K rows high, K * NB pixels wide) per
// thread; V16 (K * NB == 4, and the launcher found W % 4 == 0 and the pointers aligned): its rows in 16-byte accesses ----------
template <int K, int NB, bool V16, bool AUG>
__global__ void restore_measure_pool_kernel(const float* __restrict__ u, const float* __restrict__ eps,
                                            const float* __restrict__ y, const psld_restore_coeffs_t q, long long batch,
                                            long long c, long long h, long long w, float* __restrict__ g,
                                            float* __restrict__ cot) {
    constexpr int ROW = K * NB;
    const long long hb = h / K, wb = w / K, ws = w / ROW, hw = h * w;
    const long long n = batch * c * hb * ws;
    const double a = 1.0 / K;
    GRID_STRIDE(i, n) {
        const long long js = i % ws, bi = (i / ws) % hb, pl = i / (ws * hb);      // pl = b * c + ch
        const long long b = pl / c, ch = pl - b * c;
        const long long ox0 = ((AUG ? b * 2 * c + ch : pl) * h + bi * K) * w + js * ROW;
        const long long og0 = (pl * h + bi * K) * w + js * ROW;
        double acc[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[nb] = 0.0;
#pragma unroll
        for (int r = 0; r < K; ++r) {
            double x0[ROW];
            rs_x0<ROW, AUG, V16>(u, eps, q, ox0 + r * w, ox0 + r * w + c * hw, x0);
#pragma unroll
            for (int e = 0; e < ROW; ++e) acc[e / K] = acc[e / K] + x0[e];
        }
        double gv[ROW];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const double gb = a * ((double)y[(pl * hb + bi) * wb + js * NB + nb] - a * acc[nb]);
#pragma unroll
            for (int e = 0; e < K; ++e) gv[nb * K + e] = gb;
        }
#pragma unroll
        for (int r = 0; r < K; ++r) rs_put<ROW, AUG, V16>(g, cot, q, og0 + r * w, ox0 + r * w, ox0 + r * w + c * hw, gv);
    }
}

// ---- combine: eps^' = eps^ - kappa (q_e g - L^T dx) ---------------------------------------------------------------------
template <int VEC, bool AUG>
__device__ __forceinline__ void combine_at(const float* __restrict__ eps, const float* __restrict__ g,
                                           const float* __restrict__ dx, const psld_restore_coeffs_t& q, long long og,
                                           long long ox, long long om, float* __restrict__ out) {
    float ex[VEC], gv[VEC], dxx[VEC];
    double nx[VEC];
    rs_read<VEC>(eps + ox, ex);
    rs_read<VEC>(g + og, gv);
    rs_read<VEC>(dx + ox, dxx);
    if constexpr (AUG) {
        float em[VEC], dxm[VEC];
        double nm[VEC];
        rs_read<VEC>(eps + om, em);
        rs_read<VEC>(dx + om, dxm);
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            nx[e] = (double)ex[e] - q.kappa * ((q.q_e[0] * (double)gv[e] - q.l[0] * (double)dxx[e]) - q.l[1] * (double)dxm[e]);
            nm[e] = (double)em[e] - q.kappa * (q.q_e[1] * (double)gv[e] - q.l[2] * (double)dxm[e]);
        }
        rs_write<VEC>(out + ox, nx);
        rs_write<VEC>(out + om, nm);
    } else {
#pragma unroll
        for (int e = 0; e < VEC; ++e)
            nx[e] = (double)ex[e] - q.kappa * (q.q_e[0] * (double)gv[e] - q.l[0] * (double)dxx[e]);
        rs_write<VEC>(out + ox, nx);
    }
}

// the segments of restore_measure_mask_kernel
template <int VEC, bool AUG>
__global__ void restore_combine_kernel(const float* __restrict__ eps, const float* __restrict__ g,
                                       const float* __restrict__ dx, const psld_restore_coeffs_t q, long long nseg,
                                       long long seg, long long stride, float* __restrict__ out) {
    const long long pv = seg / VEC, nvec = nseg * pv;
    GRID_STRIDE(i, nvec) {
        const long long s = i / pv, r = (i - s * pv) * VEC;
        const long long ox = s * stride + r;
        combine_at<VEC, AUG>(eps, g, dx, q, s * seg + r, ox, ox + seg, out);
    }
    if constexpr (VEC > 1) {
        const long long tail = seg - pv * VEC, ntail = nseg * tail;
        GRID_STRIDE(i, ntail) {
            const long long s = i / tail, r = pv * VEC + (i - s * tail);
            const long long ox = s * stride + r;
            combine_at<1, AUG>(eps, g, dx, q, s * seg + r, ox, ox + seg, out);
        }
    }
}

template <int K, int NB, bool V16>
void launch_pool(bool aug, const float* u, const float* eps, const float* y, const psld_restore_coeffs_t& q, int batch,
                 int c, int h, int w, float* g, float* cot, hipStream_t stream) {
    const long long n = (long long)batch * c * (h / K) * (w / (K * NB));
    if (aug)
        hipLaunchKernelGGL((restore_measure_pool_kernel<K, NB, V16, true>), dim3(grid_for(n)), dim3(256), 0, stream, u, eps, y, q,
                           (long long)batch, (long long)c, (long long)h, (long long)w, g, cot);
    else
        hipLaunchKernelGGL((restore_measure_pool_kernel<K, NB, V16, false>), dim3(grid_for(n)), dim3(256), 0, stream, u, eps, y, q,
                           (long long)batch, (long long)c, (long long)h, (long long)w, g, cot);
}

}  // namespace

extern "C" int psld_restore_measure_f32(const float* u, const float* eps, const float* y, const float* mask, int op, int k,
                                        const psld_restore_coeffs_t* q, int batch, int c, int h, int w, float* g,
                                        float* cot, hipStream_t stream) {
    PSLD_CHECK_ARG(u && eps && y && q && g && cot && batch > 0 && c > 0 && h > 0 && w > 0,
                   "psld_restore_measure_f32: bad args");
    PSLD_CHECK_ARG(q->augmented == 0 || q->augmented == 1, "psld_restore_measure_f32: augmented %d not 0 / 1", q->augmented);
    PSLD_CHECK_ARG(op == PSLD_RESTORE_MASK || op == PSLD_RESTORE_GRAY || op == PSLD_RESTORE_POOL,
                   "psld_restore_measure_f32: operator code %d not 0 (mask) / 1 (gray) / 2 (pool)", op);
    const bool aug = q->augmented == 1;
    const long long hw = (long long)h * w, plane = (long long)c * hw;
    bool aligned = ((uintptr_t)u | (uintptr_t)eps | (uintptr_t)y | (uintptr_t)g | (uintptr_t)cot) % 16 == 0;
    if (op == PSLD_RESTORE_MASK) {
        PSLD_CHECK_ARG(mask, "psld_restore_measure_f32: the mask operator needs a mask");
        aligned = aligned && (uintptr_t)mask % 16 == 0;
        if (aug) {
            if (aligned && plane % 4 == 0)
                hipLaunchKernelGGL((restore_measure_mask_kernel<4, true>), dim3(grid_for(batch * plane / 4)), dim3(256), 0,
                                   stream, u, eps, y, mask, *q, (long long)batch, plane, 2 * plane, g, cot);
            else
                hipLaunchKernelGGL((restore_measure_mask_kernel<1, true>), dim3(grid_for(batch * plane)), dim3(256), 0,
                                   stream, u, eps, y, mask, *q, (long long)batch, plane, 2 * plane, g, cot);
        } else {
            const long long n = batch * plane;
            if (aligned && n >= 4)
                hipLaunchKernelGGL((restore_measure_mask_kernel<4, false>), dim3(grid_for(n / 4)), dim3(256), 0, stream, u,
                                   eps, y, mask, *q, 1LL, n, n, g, cot);
            else
                hipLaunchKernelGGL((restore_measure_mask_kernel<1, false>), dim3(grid_for(n)), dim3(256), 0, stream, u, eps,
                                   y, mask, *q, 1LL, n, n, g, cot);
        }
    } else if (op == PSLD_RESTORE_GRAY) {
        PSLD_CHECK_ARG(c == 3, "psld_restore_measure_f32: the gray operator needs 3 channels, got %d", c);
        const double a = 1.0 / sqrt(3.0);
        const bool vec = aligned && hw % 4 == 0;
        const long long n = vec ? batch * hw / 4 : batch * hw;
        if (vec && aug)
            hipLaunchKernelGGL((restore_measure_gray_kernel<4, true>), dim3(grid_for(n)), dim3(256), 0, stream, u, eps, y, *q,
                               a, (long long)batch, hw, g, cot);
        else if (vec)
            hipLaunchKernelGGL((restore_measure_gray_kernel<4, false>), dim3(grid_for(n)), dim3(256), 0, stream, u, eps, y,
                               *q, a, (long long)batch, hw, g, cot);
        else if (aug)
            hipLaunchKernelGGL((restore_measure_gray_kernel<1, true>), dim3(grid_for(n)), dim3(256), 0, stream, u, eps, y, *q,
                               a, (long long)batch, hw, g, cot);
        else
            hipLaunchKernelGGL((restore_measure_gray_kernel<1, false>), dim3(grid_for(n)), dim3(256), 0, stream, u, eps, y,
                               *q, a, (long long)batch, hw, g, cot);
    } else {
        PSLD_CHECK_ARG(k == 2 || k == 4, "psld_restore_measure_f32: pool block size %d not 2 / 4", k);
        PSLD_CHECK_ARG(h % k == 0 && w % k == 0, "psld_restore_measure_f32: map %d x %d is no multiple of the pool block %d",
                       h, w, k);
        // 16-byte rows: every row of a strip starts at a multiple of 4 elements when W % 4 == 0
        const bool vec = aligned && w % 4 == 0;
        if (k == 4) {
            if (vec) launch_pool<4, 1, true>(aug, u, eps, y, *q, batch, c, h, w, g, cot, stream);
            else launch_pool<4, 1, false>(aug, u, eps, y, *q, batch, c, h, w, g, cot, stream);
        } else {
            if (vec) launch_pool<2, 2, true>(aug, u, eps, y, *q, batch, c, h, w, g, cot, stream);
            else launch_pool<2, 1, false>(aug, u, eps, y, *q, batch, c, h, w, g, cot, stream);
        }
    }
    PSLD_CHECK_LAUNCH("psld_restore_measure_f32");
    return PSLD_OK;
}

extern "C" int psld_restore_combine_f32(const float* eps, const float* g, const float* dx, const psld_restore_coeffs_t* q,
                                        int batch, int c, int hw, float* out, hipStream_t stream) {
    PSLD_CHECK_ARG(eps && g && dx && q && out && batch > 0 && c > 0 && hw > 0, "psld_restore_combine_f32: bad args");
    PSLD_CHECK_ARG(q->augmented == 0 || q->augmented == 1, "psld_restore_combine_f32: augmented %d not 0 / 1", q->augmented);
    const bool aligned = ((uintptr_t)eps | (uintptr_t)g | (uintptr_t)dx | (uintptr_t)out) % 16 == 0;
    const long long plane = (long long)c * hw;
    if (q->augmented) {
        if (aligned && plane % 4 == 0)
            hipLaunchKernelGGL((restore_combine_kernel<4, true>), dim3(grid_for(batch * plane / 4)), dim3(256), 0, stream, eps,
                               g, dx, *q, (long long)batch, plane, 2 * plane, out);
        else
            hipLaunchKernelGGL((restore_combine_kernel<1, true>), dim3(grid_for(batch * plane)), dim3(256), 0, stream, eps, g,
                               dx, *q, (long long)batch, plane, 2 * plane, out);
    } else {
        const long long n = batch * plane;
        if (aligned && n >= 4)
            hipLaunchKernelGGL((restore_combine_kernel<4, false>), dim3(grid_for(n / 4)), dim3(256), 0, stream, eps, g, dx, *q,
                               1LL, n, n, out);
        else
            hipLaunchKernelGGL((restore_combine_kernel<1, false>), dim3(grid_for(n)), dim3(256), 0, stream, eps, g, dx, *q,
                               1LL, n, n, out);
    }
    PSLD_CHECK_LAUNCH("psld_restore_combine_f32");
    return PSLD_OK;
}
