// Class conditioning and classifier-free guidance: the label embedding added to the time embedding, its table gradient,
// and the guidance combine of the conditional and unconditional halves of one batched network call.
// All three are bandwidth-trivial ([B][4*nf] and [B][C][H][W] tensors): plain loads and stores.
#include "common.h"
#include "psld_hip.h"

namespace {

#define GRID_STRIDE(i, n) \
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

// row of the table sample i reads: the "no label" row where its drop flag is set
__device__ __forceinline__ long long label_row(const long long* __restrict__ labels, const unsigned char* __restrict__ drop,
                                               int i, int null_row) {
    return (drop && drop[i]) ? (long long)null_row : labels[i];
}

// temb[i][:] += table[lab_i][:]; V floats per thread (4: d % 4 == 0 and 16-byte aligned pointers).  A label outside the
// table (a contract violation, asserted by the caller) adds nothing instead of reading past it.
template <int V>
__global__ void label_embed_add_kernel(float* __restrict__ temb, const float* __restrict__ table,
                                       const long long* __restrict__ labels, const unsigned char* __restrict__ drop,
                                       int batch, int d, int n_rows, int null_row) {
    const int dv = d / V;
    const long long n = (long long)batch * dv;
    GRID_STRIDE(i, n) {
        const int row = (int)(i / dv);
        const int col = (int)(i - (long long)row * dv);
        const long long lab = label_row(labels, drop, row, null_row);
        if (lab < 0 || lab >= n_rows) continue;
        if (V == 4) {
            f32x4* dst = reinterpret_cast<f32x4*>(temb + (long long)row * d) + col;
            *dst = *dst + reinterpret_cast<const f32x4*>(table + lab * d)[col];
        } else {
            temb[(long long)row * d + col] += table[lab * d + col];
        }
    }
}

// dtable[r][:] = sum over the samples i with lab_i == r of dtemb[i][:], in sample order (no atomics: two runs are bitwise
// equal); a row nobody selects gets zeros.  One workgroup per (row, 256 columns): it stages the labels in LDS once per 1024
// samples and every thread walks them for its own column.
constexpr int LABEL_CHUNK = 1024;
__global__ void label_embed_grad_kernel(const float* __restrict__ dtemb, const long long* __restrict__ labels,
                                        const unsigned char* __restrict__ drop, int batch, int d, int null_row,
                                        float* __restrict__ dtable, int accumulate) {
    __shared__ int slab[LABEL_CHUNK];
    const int r = blockIdx.x;
    const int col = blockIdx.y * blockDim.x + threadIdx.x;
    float acc = 0.f;
    for (int base = 0; base < batch; base += LABEL_CHUNK) {
        const int cnt = min(LABEL_CHUNK, batch - base);
        __syncthreads();
        for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
            const long long lab = label_row(labels, drop, base + j, null_row);
            slab[j] = (lab < 0 || lab > 0x7fffffffLL) ? -1 : (int)lab;
        }
        __syncthreads();
        if (col < d)
            for (int j = 0; j < cnt; ++j)
                if (slab[j] == r) acc += dtemb[(long long)(base + j) * d + col];
    }
    if (col < d) {
        float* out = dtable + (long long)r * d + col;
        *out = accumulate ? *out + acc : acc;
    }
}

// out = u + s * (c - u) over the halves c = eps2[0:n], u = eps2[n:2n]
template <int V>
__global__ void cfg_combine_kernel(const float* __restrict__ eps2, float s, float* __restrict__ out, long long n) {
    const long long nv = n / V;
    GRID_STRIDE(i, nv) {
        if (V == 4) {
            const f32x4 c = reinterpret_cast<const f32x4*>(eps2)[i];
            const f32x4 u = reinterpret_cast<const f32x4*>(eps2 + n)[i];
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = __fmaf_rn(s, c[k] - u[k], u[k]);
            reinterpret_cast<f32x4*>(out)[i] = o;
        } else {
            const float u = eps2[n + i];
            out[i] = __fmaf_rn(s, eps2[i] - u, u);
        }
    }
}

inline bool aligned16(const void* a, const void* b, const void* c = nullptr) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

}  // namespace

extern "C" int psld_label_embed_add_f32(float* temb, const float* table, const long long* labels, const unsigned char* drop,
                                        int batch, int d, int n_rows, int null_row, hipStream_t stream) {
    PSLD_CHECK_ARG(temb && table && labels && batch > 0 && d > 0 && n_rows > 0 && null_row >= 0 && null_row < n_rows,
                   "psld_label_embed_add_f32: bad args");
    if (d % 4 == 0 && aligned16(temb, table)) {
        hipLaunchKernelGGL(label_embed_add_kernel<4>, dim3(psld_grid_blocks((long long)batch * (d / 4), 256, 4096)), dim3(256),
                           0, stream, temb, table, labels, drop, batch, d, n_rows, null_row);
    } else {
        hipLaunchKernelGGL(label_embed_add_kernel<1>, dim3(psld_grid_blocks((long long)batch * d, 256, 4096)), dim3(256), 0,
                           stream, temb, table, labels, drop, batch, d, n_rows, null_row);
    }
    PSLD_CHECK_LAUNCH("psld_label_embed_add_f32");
    return PSLD_OK;
}

extern "C" int psld_label_embed_grad_f32(const float* dtemb, const long long* labels, const unsigned char* drop, int batch,
                                         int d, int n_rows, int null_row, float* dtable, int accumulate, hipStream_t stream) {
    PSLD_CHECK_ARG(dtemb && labels && dtable && batch > 0 && d > 0 && n_rows > 0 && null_row >= 0 && null_row < n_rows &&
                       cdiv(d, 256) <= 65535,
                   "psld_label_embed_grad_f32: bad args");
    hipLaunchKernelGGL(label_embed_grad_kernel, dim3(n_rows, cdiv(d, 256)), dim3(256), 0, stream, dtemb, labels, drop, batch,
                       d, null_row, dtable, accumulate);
    PSLD_CHECK_LAUNCH("psld_label_embed_grad_f32");
    return PSLD_OK;
}

extern "C" int psld_cfg_combine_f32(const float* eps2, float scale, float* out, long long n, hipStream_t stream) {
    PSLD_CHECK_ARG(eps2 && out && n > 0, "psld_cfg_combine_f32: bad args");
    if (n % 4 == 0 && aligned16(eps2, out)) {
        hipLaunchKernelGGL(cfg_combine_kernel<4>, dim3(psld_grid_blocks(n / 4, 256, 4096)), dim3(256), 0, stream, eps2, scale,
                           out, n);
    } else {
        hipLaunchKernelGGL(cfg_combine_kernel<1>, dim3(psld_grid_blocks(n, 256, 4096)), dim3(256), 0, stream, eps2, scale, out,
                           n);
    }
    PSLD_CHECK_LAUNCH("psld_cfg_combine_f32");
    return PSLD_OK;
}
