// Winograd F(2x2, 3x3) form of the 3x3 stride-1 pad-1 convolutions (forward and data gradient) on the bf16 limb MFMA
// path of conv_split.hip: 2.25x fewer matrix instructions for the same fp32-equivalent result.
//
//   Y = A^T [ (G g G^T) (.) (B^T d B) ] A        d: 4x4 input tile, g: 3x3 filter, Y: 2x2 output tile (Lavin & Gray)
//
// It is a re-association of the same fp32 arithmetic, not a narrower one: the transformed operands V = B^T d B and
// U = G g G^T are formed in fp32, each is decomposed EXACTLY into three bf16 limbs (limb.h: split3) and every product
// is accumulated in fp32 from the six limb products of weight >= 2^-16, as in the direct kernels.  What the reference's
// GPU path may run for exactly these layers (nn.Conv2d 3x3 fp32 -> cuDNN Winograd; song_sde/layers.py:103-109).
//
// Shape of the kernel (one 512-thread workgroup per CU, two waves per SIMD):
//   * a workgroup owns 32 tiles (= 128 consecutive output pixels, the direct kernel's tile) x 128 output channels for
//     ALL 16 transform positions; wave w owns the 16 channels n0 + 16w.. for the 32 tiles: 16 positions x 2 tile blocks
//     of v_mfma_f32_16x16x32_bf16 accumulators = 128 VGPRs, so the output transform A^T m A is register arithmetic in
//     the lane that holds (tile, 4 channels) - no exchange between waves;
//   * per 32-channel chunk the raw fp32 halo tile ((rows+2) x (W+2) pixels, <= 36 KB) goes global -> registers (loaded
//     a whole MFMA phase ahead) -> LDS; every thread then transforms (tile, 4 channels, 8 of the 16 positions):
//     2 adds per V element, split3, and writes the limb image V[pos][limb][tile][32 ch] (96 KB) - the split is paid
//     once per V element and workgroup;
//   * U comes pre-transformed and pre-split in MFMA operand order (psld_pack_conv3x3_wino, once per optimizer step,
//     16/9 the bytes of the direct fragments) straight from L2, each fragment loaded by exactly one wave;
//   * per chunk and wave: 16 positions x (6 ds_read_b128 + 3 global loads + 12 MFMAs).
// Epilogue = the direct kernels' (bias / time-embedding row bias / residual / scale / accumulate / GroupNorm partial
// sums of the output), applied to the four output pixels of a tile.
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "common.h"
#include "psld_hip.h"
#include "tile_shared.h"
#include "limb.h"

namespace {

constexpr int WT = 32;                    // tiles per workgroup
constexpr int VPLANE = WT * ROWB;         // bytes of one (position, limb) plane of the V image: 32 tiles x 64 B
constexpr int VBYTES = 16 * 3 * VPLANE;   // 98,304 (three limbs; two: 65,536; one fp16 plane: 32,768)
constexpr int WINO_THREADS = 512;

struct WinoArgs {
    const float* x1;
    const float* x2;
    int C1, C2;
    int B, H, W;
    const u32x4* ufrag;     // [N/16 = 128-channel tile x 8 waves][chunk][16 pos][3 limbs][64 lanes] (a tail tile: fewer waves; NL = 2 / 1: two limbs / one fp16 plane)
    int N, M;               // cout (multiple of 128; TAIL: of 32, >= 128 - the last channel tile is cut short), B*H*W
    int chunks;             // (C1 + C2) / 32
    float* C;
    int ldc;
    int nseg, rps;          // image segments per 128-pixel tile and output rows per segment (dconv_geometry, mt = 128)
    int cw;                 // wino_conv8s_kernel: width of a workgroup's pixel block (W, or 32 on 64- and 128-wide maps: rps = 4)
    PsldEpilogue e;
    const float* zero;
    int nmajor;
    int tiles_m;            // pixel tiles of the launch, cdiv(M, 128): the grid is ksplit x tiles_m x channel tiles (launch_wino8s)
    int stagger;
    // wino_conv8s_kernel<., GNF = true>: GroupNorm apply (+ SiLU) of the input inside the raw staging - per-(image, channel)
    // scale / shift rows of source 1 and 2 ([B][C1], [B][C2]: psld_gn_stats_*), act = 1: SiLU
    const float *gsc1, *gsh1, *gsc2, *gsh2;
    int gn_act;
    unsigned long long* dbg;    // ablation library: s_memtime stamps of one chunk (ABL & 64), [workgroup][wave][8]
    int lg_tiles_x, lg_tps; // log2 of the tiles per tile row (cw / 2) and per image segment
    // wino_conv8s_kernel, small grids (round 6): the channel chunks split over ksplit workgroups per tile, each writing its plain
    // partial output to C + split * slab_stride (no epilogue); psld_detail_conv_reduce_epilogue sums them.  ksplit = 0 / 1: off
    int ksplit;
    long long slab_stride;
    // wino_conv8s_kernel: the launch geometry's divisions, done once on the host (wino_conv).  Powers of two as
    // their log2; the halo decomposition px -> (seg, hr, hx), px < 256, as exact multiply-shifts (wino_div16)
    int lg_ksplit, lg_xblocks;  // log2 of ksplit (0: off) and of W / cw
    int lg_rpi;                 // log2 of the regions per image (H * W / 128), -1: not a power of two (non-square maps)
    int mul_seg, mul_w2;        // wino_div16 multipliers of seg_px = (rps + 2) * (cw + 2) and of W2 = cw + 2
    int rb_img;                 // the row bias is one row per image (rows_per_img == H * W): its row is the image index
    float opscale;              // wino_conv8s_kernel<..., NL = 1, SH = true>: V is multiplied by this power of two before it is rounded to fp16
};

// x / d for 0 <= x < 256 as (x * wino_mul16(d)) >> 16: exact for every divisor the halo decomposition meets
constexpr int wino_mul16(int d) { return 65536 / d + 1; }
__host__ __device__ constexpr int wino_div16(int x, int mul) { return (x * mul) >> 16; }
// every (rps, cw) wino_geometry returns (64- and 128-wide maps run as the 32-wide case); nseg * seg_px <= 256
constexpr int WINO_GEOS[7][2] = {{4, 4}, {4, 8}, {8, 8}, {16, 8}, {4, 16}, {8, 16}, {4, 32}};
constexpr bool wino_div16_exact() {
    for (const auto& g : WINO_GEOS) {
        const int W2 = g[1] + 2, seg_px = (g[0] + 2) * W2;
        for (int x = 0; x < 256; ++x)
            if (wino_div16(x, wino_mul16(seg_px)) != x / seg_px || wino_div16(x, wino_mul16(W2)) != x / W2) return false;
    }
    return true;
}
static_assert(wino_div16_exact(), "halo decomposition: multiply-shift must equal the division for every pixel below 256");
constexpr bool wino_geo_listed(int rps, int cw) {
    for (const auto& g : WINO_GEOS)
        if (g[0] == rps && g[1] == cw) return true;
    return false;
}
constexpr int wino_lg2(int v) {     // log2 of a power of two, -1 otherwise
    int l = 0;
    while ((1 << l) < v) ++l;
    return (1 << l) == v ? l : -1;
}

// raw halo image: pixel hp, 16-byte slot q (4 channels) -> byte offset.  Pixels sit pairwise in 256-byte rows and the
// half of the row a pixel takes alternates with the pair index: the transform phase reads pixels 2 apart (tiles are two
// pixels wide), which a linear [pixel][128 B] image would put on half of the banks (2-way conflict on ds_read_b128).
__device__ __forceinline__ int raw_off(int hp, int q) {
    return (hp >> 1) * 256 + (((((hp & 1) ^ ((hp >> 1) & 1)) << 3) + q) << 4);
}

// ---- weights -> transformed limb fragments -----------------------------------------------------------------
// One work item = lane slot (nt, wave, chunk, lane): n = nt*128 + wave*16 + (lane & 15), k = chunk*32 + (lane >> 4)*8 + j.
// dgrad = 0: g = w[co = n][ci = k][:, :]; dgrad = 1: g = w[co = k][ci = n] rotated by 180 degrees (conv_split.hip).
// NL = 2 (PSLD_MATH_BF16X3): the hi and mid limbs only, [...][16 pos][2 limbs][64 lanes] - bit for bit planes 0 and 1 of NL = 3.
// NL = 1 (eval math f16): U rounded once to fp16 (limb.h: cvt_pk_f16), [...][16 pos][1][64 lanes].
template <int NL = 3>
__device__ __forceinline__ void wino_pack_item(const float* __restrict__ w, u32x4* __restrict__ out, long long it, int k_in,
                                               long long sn, long long sk, int flip) {
    const int chunks = k_in / 32;
    long long t = it;
    const int lane = (int)(t & 63); t >>= 6;
    const int chunk = (int)(t % chunks); t /= chunks;
    const int nblk = (int)t;                            // nt*8 + wave
    const int n = nblk * 16 + (lane & 15);
    const int k0 = chunk * 32 + (lane >> 4) * 8;
    float U[8][16];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float* p = w + n * sn + (k0 + j) * sk;
        float g[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = flip ? p[8 - (a * 3 + b)] : p[a * 3 + b];
        float t4[4][3];                                 // G g
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            t4[0][b] = g[0][b];
            t4[1][b] = 0.5f * ((g[0][b] + g[2][b]) + g[1][b]);
            t4[2][b] = 0.5f * ((g[0][b] + g[2][b]) - g[1][b]);
            t4[3][b] = g[2][b];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {                   // (G g) G^T
            U[j][a * 4 + 0] = t4[a][0];
            U[j][a * 4 + 1] = 0.5f * ((t4[a][0] + t4[a][2]) + t4[a][1]);
            U[j][a * 4 + 2] = 0.5f * ((t4[a][0] + t4[a][2]) - t4[a][1]);
            U[j][a * 4 + 3] = t4[a][2];
        }
    }
    u32x4* o = out + ((long long)nblk * chunks + chunk) * (16 * NL * 64) + lane;
#pragma unroll
    for (int p = 0; p < 16; ++p) {
        unsigned hi[4], mid[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (NL == 3) split3(U[2 * j][p], U[2 * j + 1][p], hi[j], mid[j], lo[j]);
            else if constexpr (NL == 2) split2(U[2 * j][p], U[2 * j + 1][p], hi[j], mid[j]);
            else hi[j] = cvt_pk_f16(U[2 * j][p], U[2 * j + 1][p]);
        }
        o[(p * NL + 0) * 64] = u32x4{hi[0], hi[1], hi[2], hi[3]};
        if constexpr (NL >= 2) o[(p * NL + 1) * 64] = u32x4{mid[0], mid[1], mid[2], mid[3]};
        if constexpr (NL == 3) o[(p * 3 + 2) * 64] = u32x4{lo[0], lo[1], lo[2], lo[3]};
    }
}

template <int NL = 3>
__global__ void wino_pack_kernel(const float* __restrict__ w, u32x4* __restrict__ out, int n_out, int k_in,
                                 long long sn, long long sk, int flip) {
    const long long items = (long long)(n_out / 16) * (k_in / 32) * 64;
    for (long long it = (long long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long long)gridDim.x * blockDim.x)
        wino_pack_item<NL>(w, out, it, k_in, sn, sk, flip);
}

// Many weight tensors in one launch (as pack_frag_batch_kernel of conv_split.hip).  tab[8*i ..]: src pointer, dst
// pointer, n_out, k_in, flip, sn, sk, first work item of tensor i (a tensor has n_out * k_in / 8 items).
template <int NL = 3>
__global__ void wino_pack_batch_kernel(const long long* __restrict__ tab, int ntab, long long total) {
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        int lo = 0, hi = ntab - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (tab[8 * mid + 7] <= idx) lo = mid; else hi = mid - 1;
        }
        const long long* d = tab + 8 * lo;
        wino_pack_item<NL>(reinterpret_cast<const float*>(d[0]), reinterpret_cast<u32x4*>(d[1]), idx - d[7], (int)d[3], d[5], d[6],
                       (int)d[4]);
    }
}

// ---- eight waves, staggered roles: the transform of one SIMD partner runs under the MFMAs of the other ----------------
// Same tile, same wave tile as wino_conv_kernel (wave w: 32 tiles x 16 channels x 16 positions, 128 accumulator VGPRs,
// two waves per SIMD) and the half-image schedule of wino_conv4_kernel (HP0(c): MFMAs on V rows 0,1 of chunk c, V rows 2,3
// of chunk c being produced; HP1(c): MFMAs on rows 2,3, rows 0,1 of chunk c + 1 being produced; one barrier after each).
// Inside a half-phase every wave has two blocks of work - its share of the transform (one V row of one (tile, channel
// quad) item: 8 ds_read_b128, 32 adds, 8 split3 pairs, 12 ds_write_b64) and 8 positions x 12 MFMAs - and the two waves
// that share a SIMD (w and w + 4) run them in OPPOSITE order: while one issues vector ALU work the other owns the matrix
// pipe, with no instruction-level interleaving to get right (the hardware arbitrates between the two waves) and the
// partner's MFMAs covering each wave's memory latencies, which one wave per SIMD has to cover by itself.
// (Output tile through LDS so that every wave stores whole 512-byte pixel rows instead of 64-byte runs: built, correct,
// 2.5 % slower - 454 vs 443 us - although skipping the stores altogether saves 8 %: the exposed part of the epilogue is the
// drain of 64 KB per workgroup, not the segment size.)
// (Two persistent forms of this kernel were built and measured slower: workgroups walking (pixel tile, channel tile) work
// lists, 480 vs 454 us on 256->256 @32x32 B=128, and one workgroup per pixel tile looping over the channel tiles with the
// half-phase pipeline running across the passes, 522 vs 451 us - hipcc's code for the accumulators degrades once the
// epilogue sits inside a loop.  One workgroup per (pixel tile, channel tile) it is.  Both tried to HIDE a workgroup's ends - the
// set-up and the epilogue, ~13 us that nothing covers on a CU the workgroup has to itself - behind a neighbouring item; the
// epilogue's vector instructions are zero-sum beside a partner's MFMAs.  The ends are SHORTENED instead: no runtime division in
// the index arithmetic (WinoArgs carries shifts and multiply-shift constants), the last chunk peeled out of the loop without the
// staging and transform of a chunk that does not exist, A^T m A in place with 32-bit offsets from scalar bases.  profiles/r08/README.md has the per-launch times against the previous kernel.)
// GNF: the input is the RAW tensor a GroupNorm (+ SiLU) is to be applied to, and the apply pass runs here, on the float4 a
// thread has just loaded for the raw image: a = silu(x * scale[img][c] + shift[img][c]), zero outside the image (the
// convolution pads the ACTIVATED tensor).  The inference forward (EM / SSCS sampling) needs the activated tensor nowhere
// else, so psld_gn_apply_nhwc_f32's round trip through HBM disappears; one image per region only (maps of >= 128 pixels).
// The scale / shift quad is loaded where it is used (L1 / L2 hits; holding it in registers through the MFMA phase, or
// staging it through LDS two half-phases ahead, spills: the kernel sits at 256 VGPRs).  Measured (profiles/r04/
// wino_fused_gn.txt): the launch gets 7-10 % longer - ~110 vector instructions per thread and chunk, two of them
// transcendental per element, in a kernel that is short of vector issue slots - against the apply pass it replaces: 3-5 %
// less time for the pair on the 32x32 level at B=512, nothing on 16x16.  Reference: GroupNorm_0/1 + act in front of
// Conv_0/1, layerspp.py:245-263.
// ERAW: the raw halo of chunk c + 1 is requested right after the MFMAs of HP1(c - 1) instead of at the head of HP0(c).
// Vector-memory operations retire in issue order (one vmcnt): at the head of HP0 the four halo loads (HBM latency) sit in
// front of every weight-fragment load of the half-phase, and the first s_waitcnt of the MFMA stream waits for them.
// Issued behind the last fragment wait of the previous half-phase they have that phase's transform and the barrier to
// land before anything younger is waited for.
// TAIL (cout % 128 != 0 only): the last channel tile holds 32, 64 or 96 channels; the waves beyond cout take their share of the
// staging and the transform (and the barriers) but load no fragments, issue no MFMAs and leave before the epilogue.  Every
// live wave does exactly what it does in a full tile, so a channel's result does not depend on how many share its launch.
// NL = 2 (PSLD_MATH_BF16X3; the data gradient is this kernel on dgrad = 1 fragments): V and U keep their first two limbs (split2) and a product is the three limb
// products hi*hi + (hi*lo + lo*hi): V image [pos][2][tile][32 ch] (64 KB), fragments [...][16 pos][2 limbs][64 lanes], per
// chunk and wave 16 positions x (4 ds_read_b128 + 2 fragment loads + 6 MFMAs).  Everything else is the NL = 3 kernel.
// NL = 1 (eval math f16, forward only): V and U are rounded ONCE to fp16 (cvt_pk_f16: round to nearest even, clamped to +-65504)
// and a product is one v_mfma_f32_16x16x32_f16 - exact in fp32 (11 + 11 significant bits), so the operand rounding is the mode's
// only error.  V image [pos][1][tile][32 ch] (32 KB), fragments [...][16 pos][1][64 lanes], per chunk and wave 16 positions x
// (2 ds_read_b128 + 1 fragment load + 2 MFMAs).  fp32 transforms, accumulation, output transform and epilogue are the NL = 3 kernel's.
// SH (NL = 1 only; record f16: the data gradient is this kernel on dgrad = 1 fragments): V is multiplied by a.opscale = 2^shift in
// fp32 - exact - before the one rounding, so that gradients of a mean-reduced loss (~2/N, fp16 subnormals or zero) keep 11
// significant bits; the host folds 2^-shift into the epilogue's alpha.  One v_mul_f32 per V value, nothing else changes.
template <int ABL = 0, bool GNF = false, bool ERAW = false, int LA = 2, bool TAIL = false, int NL = 3, bool SH = false>
__global__ void __launch_bounds__(WINO_THREADS) wino_conv8s_kernel(const WinoArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NI = 4;                     // raw image: 256 halo pixels
    constexpr int RAWB = NI * 64 * 128;
    unsigned char* Vs = smem;
    unsigned char* Rs = smem + VBYTES / 3 * NL;        // two raw images

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tiles_n = TAIL ? (a.N + 127) >> 7 : a.N >> 7;
    const int nsp = a.ksplit > 1 ? a.ksplit : 1;
    const int tiles_m = a.tiles_m;
    const int per_range = tiles_m * tiles_n;                     // workgroups of one channel-chunk range (gridDim.x / nsp)
    const int vb = xcd_remap(blockIdx.x, gridDim.x);
    const int split = nsp > 1 ? vb / per_range : 0;
    const int bid = vb - split * per_range;
    const int kch = a.chunks >> a.lg_ksplit, ch0 = split * kch;  // this workgroup's chunks [ch0, ch0 + kch)
    float* const Cw = a.C + split * a.slab_stride;
    const int tile_n = a.nmajor ? bid / tiles_m : bid % tiles_n;
    const int tile_m = a.nmajor ? bid - tile_n * tiles_m : bid / tiles_n;
    const int n0 = tile_n * 128;
    const bool live = !TAIL || n0 + wave * 16 < a.N;             // wave-uniform; always true without TAIL

    // Region of this workgroup: nseg images (maps smaller than 128 pixels) or one rps x cw block of an image - cw = W, or 32
    // for 64- and 128-wide maps, whose full-width tile (2 rows x 64, 1 row x 128) would need a 264- / 390-pixel halo where
    // the two raw images hold 256.  4x4 maps: SEVEN images (7 x 36 = 252 halo pixels; eight would need 288) - tiles 28 .. 31
    // of the workgroup belong to no image: they transform halo pixel 0 onwards and store nothing.
    const int HW = a.H * a.W;
    const int W2 = a.cw + 2;
    const int lg_tx = a.lg_tiles_x, lg_tps = a.lg_tps;          // tiles per tile row and per image segment: powers of two
    const int rpi = HW >= 128 ? HW >> 7 : 1;                    // regions per image
    const int tm_img = a.lg_rpi >= 0 ? tile_m >> a.lg_rpi : tile_m / rpi;      // wave-uniform: the scalar unit's
    const int reg = tile_m - tm_img * rpi;
    const int img0 = HW >= 128 ? tm_img : tile_m * a.nseg;
    const int oy0 = (reg >> a.lg_xblocks) * a.rps, ox0 = (reg & ((1 << a.lg_xblocks) - 1)) * a.cw;
    const float* zp = a.zero;

    const int c4 = tid & 7;
    int hoff[NI], rdst[NI];
    {
        const int seg_px = (a.rps + 2) * W2;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int px = (tid + WINO_THREADS * i) >> 3;
            const int seg = wino_div16(px, a.mul_seg);
            const int rem = px - seg * seg_px;
            const int hr = wino_div16(rem, a.mul_w2), hx = rem - hr * W2;
            const int img = img0 + seg, iy = oy0 + hr - 1, ix = ox0 + hx - 1;
            const bool ok = seg < a.nseg && img < a.B && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
            hoff[i] = ok ? (img * a.H + iy) * a.W + ix : -1;
            rdst[i] = raw_off(px, c4);
        }
    }
    f32x4 hv[NI];
    auto load_raw = [&](int c) {
        const int c0 = c * 32;
        const bool second = c0 >= a.C1;
        const float* src = second ? a.x2 : a.x1;
        const int cs = second ? a.C2 : a.C1;
        const int cc = (second ? c0 - a.C1 : c0) + c4 * 4;
#pragma unroll
        for (int i = 0; i < NI; ++i) hv[i] = ld4(hoff[i] >= 0 ? src + ((long long)hoff[i] * cs + cc) : zp);
    };
    auto store_raw = [&](int buf, int c) {
        if constexpr (GNF) {
            const int c0 = c * 32;
            const bool second = c0 >= a.C1;
            const int cs = second ? a.C2 : a.C1;
            const long long go = (long long)img0 * cs + (second ? c0 - a.C1 : c0) + c4 * 4;
            const f32x4 sc = ld4((second ? a.gsc2 : a.gsc1) + go), sh = ld4((second ? a.gsh2 : a.gsh1) + go);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float z = hv[i][e] * sc[e] + sh[e];
                    const float v = a.gn_act ? silu_f(z) : z;
                    o[e] = hoff[i] >= 0 ? v : 0.f;          // the convolution pads the ACTIVATED tensor with zeros
                }
                *reinterpret_cast<f32x4*>(Rs + buf * RAWB + rdst[i]) = o;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) *reinterpret_cast<f32x4*>(Rs + buf * RAWB + rdst[i]) = hv[i];
        }
    };

    // ---- transform share of this thread: item (tile, channel quad) = tid & 255, V row vr = wave >> 2 of the half -------------
    const int vr = wave >> 2;
    const int t_tile = (tid & 255) >> 3, t_q = tid & 7;
    int t_src;      // halo pixel of d[0][0]
    {
        const int seg = t_tile >> lg_tps, rem = t_tile & ((1 << lg_tps) - 1);
        const int ty = rem >> lg_tx, tx = rem & ((1 << lg_tx) - 1);
        t_src = seg < a.nseg ? (seg * (a.rps + 2) + 2 * ty) * W2 + 2 * tx : 0;     // (a tile of no image: 4x4 maps)
    }
    const int t_dst = t_tile * ROWB + (((t_q >> 1) ^ lds_swz(t_tile)) << 4) + (t_q & 1) * 8;
    // raw-image offsets of d[vr + k][c]: a wave's two transforms read d rows vr .. vr + 2 only.  Formed once, in front of the
    // loop AND of the peeled last chunk (left to hipcc they are hoisted per transform variant into the loop's guarded
    // pre-header, and their ingredients spilled across the loop for the last chunk)
    int t_ro[3][4];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            t_ro[k][c] = raw_off(t_src + (vr + k) * W2 + c, t_q);
            asm volatile("" : "+v"(t_ro[k][c]));
        }
    // V row 2 th + vr from two d rows: th = 0: (0: d0 - d2) (1: d1 + d2); th = 1: (2: d2 - d1) (3: d1 - d3)
    auto transform = [&](auto TH, auto VR, int rbuf) {
        constexpr int th = decltype(TH)::value, v_r = decltype(VR)::value;
        constexpr int ra_ = th == 0 ? (v_r == 0 ? 0 : 1) : (v_r == 0 ? 2 : 1);
        constexpr int rb_ = th == 0 ? 2 : (v_r == 0 ? 1 : 3);
        constexpr bool plus = th == 0 && v_r == 1;
        constexpr int vrow = 2 * th + v_r;
        const unsigned char* Rb = Rs + rbuf * RAWB;
        f32x4 ea[4], eb[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            ea[c] = *reinterpret_cast<const f32x4*>(Rb + t_ro[ra_ - v_r][c]);
            eb[c] = *reinterpret_cast<const f32x4*>(Rb + t_ro[rb_ - v_r][c]);
        }
        f32x4 r[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) r[c] = plus ? ea[c] + eb[c] : ea[c] - eb[c];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 v = j == 0 ? r[0] - r[2] : j == 1 ? r[1] + r[2] : j == 2 ? r[2] - r[1] : r[1] - r[3];
            unsigned h0, m0_, l0, h1, m1, l1;
            if constexpr (NL == 3) {
                split3(v[0], v[1], h0, m0_, l0);
                split3(v[2], v[3], h1, m1, l1);
            } else if constexpr (NL == 2) {
                split2(v[0], v[1], h0, m0_);
                split2(v[2], v[3], h1, m1);
            } else if constexpr (SH) {
                h0 = cvt_pk_f16(v[0] * a.opscale, v[1] * a.opscale);
                h1 = cvt_pk_f16(v[2] * a.opscale, v[3] * a.opscale);
            } else {
                h0 = cvt_pk_f16(v[0], v[1]);
                h1 = cvt_pk_f16(v[2], v[3]);
            }
            unsigned char* q = Vs + (vrow * 4 + j) * NL * VPLANE + t_dst;
            *reinterpret_cast<u32x2*>(q) = u32x2{h0, h1};
            if constexpr (NL >= 2) *reinterpret_cast<u32x2*>(q + VPLANE) = u32x2{m0_, m1};
            if constexpr (NL == 3) *reinterpret_cast<u32x2*>(q + 2 * VPLANE) = u32x2{l0, l1};
        }
    };

    // ---- MFMA role: 32 tiles x 16 channels x 16 positions ------------------------------------------------------------
    const int r16 = lane & 15, kq = lane >> 4;
    int aoff[2];
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
        const int row = tb * 16 + r16;
        aoff[tb] = row * ROWB + ((kq ^ lds_swz(row)) << 4);
    }
    // ABL & 128 (timing only, wrong results): SIMD partners w, w + 4 stream the SAME fragments - what the L1 merges
    const u32x4* ub = a.ufrag + ((long long)(tile_n * 8 + ((ABL & 128) ? (wave & 3) : wave)) * a.chunks + ch0) * (16 * NL * 64);      // wave-uniform
    u32x4 bq[4][NL];
    auto load_b = [&](int sigma, u32x4 (&dst)[NL]) {
        const u32x4* p = ub + (long long)sigma * (NL * 64);
#pragma unroll
        for (int l = 0; l < NL; ++l) dst[l] = p[l * 64 + lane];
    };
    f32x4v acc[16][2];
#pragma unroll
    for (int p = 0; p < 16; ++p)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) acc[p][tb] = f32x4v{0.f, 0.f, 0.f, 0.f};
    u32x4 fa[NL == 1 ? 2 : NL][2];         // [limb hi | mid | lo][tile block]; NL = 1: [position parity][tile block]
    auto read_a = [&](int p, int l) {
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) fa[l][tb] = *reinterpret_cast<const u32x4*>(Vs + (p * NL + l) * VPLANE + aoff[tb]);
    };
    auto mm = [&](int p, int la, int lb) {
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
            if constexpr (NL == 1)
                acc[p][tb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(   // one fp16 product: the bf16 operand order, element type changed
                    __builtin_bit_cast(f16x8, bq[p & 3][lb]), __builtin_bit_cast(f16x8, fa[la][tb]), acc[p][tb], 0, 0, 0);
            else
                acc[p][tb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(      // weights first: D^T[channel][tile]
                    __builtin_bit_cast(bf16x8, bq[p & 3][lb]), __builtin_bit_cast(bf16x8, fa[la][tb]), acc[p][tb], 0, 0, 0);
        }
    };
    // the eight positions of half h of chunk c (see wino_conv_kernel for the group order and the in-place A prefetch)
    // LAST (the final half-phase of the workgroup): no fragment is requested past the last position
    auto mfma_half = [&](auto HH, auto LAST, int c) {
        constexpr int h = decltype(HH)::value;
        constexpr bool last = decltype(LAST)::value;
        if constexpr ((ABL & 256) != 0) __builtin_amdgcn_s_setprio(2);       // experiment: the multiplying wave outranks its partner
        if constexpr (NL == 1) {        // one plane: position p + 1's A operand is read (other parity) in front of p's two MFMAs
            auto read_a1 = [&](int p) {
#pragma unroll
                for (int tb = 0; tb < 2; ++tb) fa[p & 1][tb] = *reinterpret_cast<const u32x4*>(Vs + p * VPLANE + aoff[tb]);
            };
            read_a1(8 * h);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int p = 8 * h + i;
                if (!(last && p + LA >= 16)) load_b(c * 16 + p + LA, bq[(p + LA) & 3]);
                if (i < 7) read_a1(p + 1);
                __builtin_amdgcn_sched_barrier(0);
                mm(p, p & 1, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            return;
        }
        // NL = 2: three products, small terms first - V_lo U_hi, V_hi U_lo, V_hi U_hi
        if constexpr (NL == 3) read_a(8 * h, 2);
        if constexpr (NL >= 2) read_a(8 * h, 1);
        read_a(8 * h, 0);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int p = 8 * h + i;
            if (!(ABL & 2) && !(last && p + LA >= 16)) load_b(c * 16 + p + LA, bq[(p + LA) & 3]);
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (NL == 3) {
                mm(p, 2, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (i < 7) read_a(p + 1, 2);
                __builtin_amdgcn_sched_barrier(0);
                mm(p, 1, 1);
            }
            if constexpr (NL >= 2) {
                mm(p, 1, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (i < 7) read_a(p + 1, 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (NL == 3) mm(p, 0, 2);
            if constexpr (NL >= 2) mm(p, 0, 1);
            mm(p, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (i < 7) read_a(p + 1, 0);
        }
        if constexpr ((ABL & 256) != 0) __builtin_amdgcn_s_setprio(0);
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    // Static priority for the second-dispatched half (waves 4-7: the arbitration loser of every SIMD pair - MI355X_MICROARCH.md,
    // "Two waves per SIMD" item 4): 454 -> 443 us on 256->256 @32x32, 206 -> 201 us on 512->256 @16x16 (ABL & 4 switches it off).
    if constexpr ((ABL & 4) == 0 && (ABL & 256) == 0) { if (vr != 0) __builtin_amdgcn_s_setprio(1); }

    load_raw(ch0);
    if (live) {
        load_b(0, bq[0]);
        load_b(1, bq[1]);
        if (LA > 2) load_b(2, bq[2]);
    }
    store_raw(0, ch0);
    if constexpr (ERAW) load_raw(ch0 + min(1, kch - 1));
    __syncthreads();
    if (vr == 0) transform(I0{}, I0{}, 0); else transform(I0{}, I1{}, 0);      // V rows 0,1 of chunk 0
    __syncthreads();

    // diagnostic build (ABL & 64): where a wave's time goes inside chunk 3 - stamps go to a buffer nothing else reads
    auto stamp = [&](int c, int idx) {
        if constexpr ((ABL & 64) != 0) {
            if (c == 3 && a.dbg) {
                __builtin_amdgcn_sched_barrier(0);
                const unsigned long long t = __builtin_amdgcn_s_memtime();
                if (lane == 0) a.dbg[((long long)blockIdx.x * 8 + wave) * 8 + idx] = t;
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    using No = std::false_type;
    using Yes = std::true_type;

    for (int c = 0; c < kch - 1; ++c) {         // every chunk but the last: it has a successor to stage and transform
        // HP0: MFMAs on V rows 0,1 of chunk c || V rows 2,3 of chunk c (raw image c & 1)
        stamp(c, 0);
        if constexpr (!ERAW) load_raw(ch0 + c + 1);
        if (vr == 0 && !(ABL & 1)) transform(I1{}, I0{}, c & 1);             // waves 0-3: transform, then MFMAs
        __builtin_amdgcn_sched_barrier(0);
        if (vr == 0) stamp(c, 1);
        if (live) mfma_half(I0{}, No{}, c);
        __builtin_amdgcn_sched_barrier(0);
        if (vr != 0) stamp(c, 1);
        if (vr != 0 && !(ABL & 1)) transform(I1{}, I1{}, c & 1);             // waves 4-7: MFMAs, then transform
        stamp(c, 2);
        store_raw((c + 1) & 1, ch0 + c + 1);
        stamp(c, 3);
        __syncthreads();
        // HP1: MFMAs on V rows 2,3 of chunk c || V rows 0,1 of chunk c + 1 (raw image (c + 1) & 1)
        stamp(c, 4);
        if (vr == 0 && !(ABL & 1)) transform(I0{}, I0{}, (c + 1) & 1);
        __builtin_amdgcn_sched_barrier(0);
        if (vr == 0) stamp(c, 5);
        if (live) mfma_half(I1{}, No{}, c);
        __builtin_amdgcn_sched_barrier(0);
        if (vr != 0) stamp(c, 5);
        if constexpr (ERAW) load_raw(ch0 + min(c + 2, kch - 1));
        if (vr != 0 && !(ABL & 1)) transform(I0{}, I1{}, (c + 1) & 1);
        stamp(c, 6);
        __syncthreads();
        stamp(c, 7);
    }
    // The last chunk, straight-line (the first one when c_in = 32): nothing follows it, so no raw image is loaded or stored, no V
    // rows 0,1 are formed, no fragment is requested past position 15 and no barrier closes it - the waves go into the output
    // transform as their own MFMAs end.  (Outside the loop: hipcc's accumulator code degrades with a "last" test inside it.)
    {
        int c = kch - 1;
        asm volatile("" : "+s"(c));     // opaque until here: the chunk's LDS addresses are formed now, not carried through the loop
        stamp(c, 0);
        if (vr == 0 && !(ABL & 1)) transform(I1{}, I0{}, c & 1);
        __builtin_amdgcn_sched_barrier(0);
        if (vr == 0) stamp(c, 1);
        if (live) mfma_half(I0{}, No{}, c);
        __builtin_amdgcn_sched_barrier(0);
        if (vr != 0) stamp(c, 1);
        if (vr != 0 && !(ABL & 1)) transform(I1{}, I1{}, c & 1);
        stamp(c, 2);
        stamp(c, 3);
        __syncthreads();
        stamp(c, 4);
        __builtin_amdgcn_sched_barrier(0);
        stamp(c, 5);                    // no transform in this half-phase: slots 5 and 6 bracket the MFMAs alone
        if (live) mfma_half(I1{}, Yes{}, c);
        __builtin_amdgcn_sched_barrier(0);
        stamp(c, 6);
        stamp(c, 7);
    }

    // ---- output transform + fused epilogue (as wino_conv_kernel) -----------------------------------------------------
    // Few registers and few vector instructions beside the accumulators: A^T m A in place (the same order of additions), one
    // scalar base per operand at the region's first pixel and 32-bit byte offsets from it (the host bounds the row strides),
    // the time-embedding row once per tile block where it is one row per image.
    if (!live) return;      // no barrier follows
    // Operands: all requested here, in front of the arithmetic.  (Requested in front of the last MFMA half-phase instead, they
    // made the 32x32 launches 1-2 % slower: profiles/r08/README.md.)  Pixels count from the region's first one (org): a tile's
    // first pixel is rel = seg * H * W + 2 ty * W + 2 tx, and a tile of an image beyond the batch reads pixel org (in range:
    // img0 < B) and stores nothing.
    const PsldEpilogue& e = a.e;
    const int cn = n0 + wave * 16 + 4 * kq;
    const int org = (img0 * a.H + oy0) * a.W + ox0;
    const f32x4v zero4 = {0.f, 0.f, 0.f, 0.f};
    const bool rb_div = e.rowbias && !a.rb_img;
    char* const c_b = reinterpret_cast<char*>(Cw + (long long)org * a.ldc);                           // wave-uniform bases
    const char* const res_b = reinterpret_cast<const char*>(e.res ? e.res + (long long)org * e.ldres : zp);
    f32x4v epi_bias, epi_tbv[2], epi_rv[2][4], epi_cv[2][4];
    int epi_rel[2];
    bool epi_ok[2];
    auto epi_rows = [&](auto TB) {        // residual and previous-output rows of the four pixels of tile block tb
        constexpr int tb = decltype(TB)::value;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int px = epi_rel[tb] + (j >> 1) * a.W + (j & 1);
            epi_rv[tb][j] = e.res ? *reinterpret_cast<const f32x4v*>(res_b + (unsigned)((px * e.ldres + cn) * 4)) : zero4;
            epi_cv[tb][j] = e.accumulate ? *reinterpret_cast<const f32x4v*>(c_b + (unsigned)((px * a.ldc + cn) * 4)) : zero4;
        }
    };
    auto epi_request = [&]() {
        epi_bias = e.bias ? *reinterpret_cast<const f32x4v*>(e.bias + cn) : zero4;
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
            const int tile = tb * 16 + r16;
            const int seg = tile >> lg_tps, rem = tile & ((1 << lg_tps) - 1);
            const int ty = rem >> lg_tx, tx = rem & ((1 << lg_tx) - 1);
            epi_ok[tb] = seg < a.nseg && img0 + seg < a.B;  // whole images only: a tile is in range or not (seg = nseg: 4x4 maps)
            epi_rel[tb] = epi_ok[tb] ? seg * HW + 2 * ty * a.W + 2 * tx : 0;
            // the row bias as one row per image: the tile's image (the region's first for a tile beyond the batch)
            epi_tbv[tb] = a.rb_img ? *reinterpret_cast<const f32x4v*>(
                                         e.rowbias + (long long)(epi_ok[tb] ? img0 + seg : img0) * e.ld_rowbias + cn)
                                   : zero4;
        }
        epi_rows(I0{});
    };
    epi_request();
    epi_rows(I1{});
    const f32x4v bias4 = epi_bias;
#pragma unroll
    for (int tb = 0; tb < 2; ++tb) {
        const bool ok = epi_ok[tb];
        const int rel = epi_rel[tb];
        // m -> m A per row of positions (columns (0 + 1 + 2), (1 - 2 - 3)), left in the accumulators of columns 0 and 1
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4v s0 = (acc[4 * i][tb] + acc[4 * i + 1][tb]) + acc[4 * i + 2][tb];
            acc[4 * i + 1][tb] = (acc[4 * i + 1][tb] - acc[4 * i + 2][tb]) - acc[4 * i + 3][tb];
            acc[4 * i][tb] = s0;
        }
        const f32x4v add4 = bias4 + epi_tbv[tb];
        f32x4v o[2][2];
#pragma unroll
        for (int ya = 0; ya < 2; ++ya)
#pragma unroll
            for (int xb = 0; xb < 2; ++xb) {
                const f32x4v y = ya == 0 ? (acc[xb][tb] + acc[4 + xb][tb]) + acc[8 + xb][tb]
                                         : (acc[4 + xb][tb] - acc[8 + xb][tb]) - acc[12 + xb][tb];
                f32x4v addv = add4;
                if (rb_div)     // a row bias of another granularity (none of the networks' launches): the row of each pixel
                    addv = bias4 + *reinterpret_cast<const f32x4v*>(
                                       e.rowbias + (long long)((org + rel + ya * a.W + xb) / e.rows_per_img) * e.ld_rowbias + cn);
                f32x4v x = y * e.alpha + addv;
                if (e.res) x += epi_rv[tb][ya * 2 + xb];
                x *= e.out_scale;
                if (e.accumulate) x += epi_cv[tb][ya * 2 + xb];
                o[ya][xb] = x;
            }
        // GroupNorm sums of the stored values in fp64 from the first addition on (v * v of an fp32 v is exact there: no
        // rounding in sum or sum of squares for a group's mean to amplify - conv_split.hip's epilogue, same reason)
        const bool gn_on = e.gn_part != nullptr;
        double gs = 0.0, gss = 0.0;
        if (ok) {
#pragma unroll
            for (int ya = 0; ya < 2; ++ya)
#pragma unroll
                for (int xb = 0; xb < 2; ++xb) {
                    const int px = rel + ya * a.W + xb;
                    if ((ABL & 8) && org + px != 0) continue;
                    *reinterpret_cast<f32x4v*>(c_b + (unsigned)((px * a.ldc + cn) * 4)) = o[ya][xb];
                    if (gn_on) {
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const double d = (double)o[ya][xb][v];
                            gs += d;
                            gss = fma(d, d, gss);
                        }
                    }
                }
        }
        if (gn_on) {
            double s1 = gs, s2 = gss;
#pragma unroll
            for (int sft = 1; sft <= 8; sft <<= 1) {
                s1 += __shfl_xor(s1, sft, 64);
                s2 += __shfl_xor(s2, sft, 64);
            }
            const double q1 = s1, q2 = s2;               // four-channel sums of this lane's quad (gn_fine = 4)
            s1 += __shfl_xor(s1, 16, 64);
            s2 += __shfl_xor(s2, 16, 64);
            // tile block tb = 64 pixels of one image = one run of the partial-sum table (any fixed partition of an image
            // into hw/64 runs serves: the consumer sums all of them): run 2 reg + tb, or image img0 + tb of a two-image region
            const int img = a.nseg == 1 ? img0 : img0 + tb, chunk = a.nseg == 1 ? 2 * reg + tb : 0, chunks = e.gn_hw >> 6;
            if (e.gn_fine == 4) {
                if ((lane & 0xf) == 0 && img < a.B) {
                    const int f = ((n0 + wave * 16) >> 2) + (lane >> 4);
                    double* pp = e.gn_part + (((long long)img * chunks + chunk) * (a.N >> 2) + f) * 2;
                    pp[0] = q1;
                    pp[1] = q2;
                }
            } else if ((lane & 0x1f) == 0 && img < a.B) {
                const int f = ((n0 + wave * 16) >> 3) + (lane >> 5);
                double* pp = e.gn_part + (((long long)img * chunks + chunk) * (a.N >> 3) + f) * 2;
                pp[0] = s1;
                pp[1] = s2;
            }
        }
    }
}

#ifdef PSLD_ABLATIONS
#include "conv_wino_abl.inc"
#endif

// pixel tiles (workgroups per channel tile and chunk range) of a launch: 128-pixel regions of the images, or for maps below 128
// pixels groups of nseg whole images - 128 pixels too except on 4x4 maps, whose groups are seven images = 112 pixels
inline int wino_tiles_m(int batch, int h, int w, int nseg) {
    return h * w >= 128 ? (int)cdiv((long long)batch * h * w, 128) : (int)cdiv(batch, nseg);
}

template <int ABL = 0, bool GNF = false, bool ERAW = false, int LA = 2, bool TAIL = false, int NL = 3, bool SH = false>
int launch_wino8s(const WinoArgs& a, hipStream_t stream, const char* name) {
    constexpr size_t LDS = (size_t)VBYTES / 3 * NL + 2 * (size_t)4 * 64 * 128;
    static_assert(LDS <= 163840, "LDS budget");
    if (int st = psld_lds_once<&wino_conv8s_kernel<ABL, GNF, ERAW, LA, TAIL, NL, SH>>(LDS, name)) return st;
    // the kernel finds its (chunk range, channel tile, pixel tile) from tiles_m and lg_ksplit, not from gridDim
    PSLD_CHECK_ARG(a.tiles_m == wino_tiles_m(a.B, a.H, a.W, a.nseg) && (1 << a.lg_ksplit) == (a.ksplit > 1 ? a.ksplit : 1),
                   "%s: launch geometry not filled in (tiles_m %d, ksplit %d)", name, a.tiles_m, a.ksplit);
    dim3 grid((unsigned)(a.tiles_m * cdiv(a.N, 128) * (a.ksplit > 1 ? a.ksplit : 1)));
    hipLaunchKernelGGL((wino_conv8s_kernel<ABL, GNF, ERAW, LA, TAIL, NL, SH>), grid, dim3(WINO_THREADS), LDS, stream, a);
    PSLD_CHECK_LAUNCH(name);
    return PSLD_OK;
}

int wino_cu_count() {
    static int n[PSLD_MAX_DEVICES] = {};      // per device (0 = not asked yet)
    int& cu = n[psld_device_slot()];
    if (cu <= 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            cu <= 0)
            cu = 256;
    }
    return cu;
}

bool wino_geometry(int h, int w, int* nseg, int* rps, int* halo_px) {
    if (w == 128) {     // 128-wide maps: 4 x 32 pixel blocks only (the 64-wide rule below, four blocks per row band)
        *nseg = 1; *rps = 4; *halo_px = 6 * 34;
        return h % 4 == 0;
    }
    if (w == 4) {       // 4x4 maps: seven images of 6 x 6 halo pixels per workgroup (252 of the raw image's 256), 28 of its 32 tiles
        *nseg = 7; *rps = 4; *halo_px = 7 * 36;
        return h == 4;
    }
    if (w != 8 && w != 16 && w != 32 && w != 64) return false;
    if (h % 2) return false;
    const int hw = h * w;
    if (hw >= 128) {
        if (hw % 128) return false;
        *nseg = 1;
        *rps = 128 / w;
    } else {
        if (128 % hw) return false;
        *nseg = 128 / hw;
        *rps = h;
    }
    if (*rps % 2) return false;
    *halo_px = *nseg * (*rps + 2) * (w + 2);
    // wino_conv8s_kernel: the halo of a workgroup's region in one 256-pixel raw image; 64-wide maps run as 4 x 32 blocks
    return w == 64 ? h % 4 == 0 : *halo_px <= 256;
}

}  // namespace

// + 16 KB: the kernels prefetch up to three positions (3 x 3 KB per 16-channel block) past the last fragment
extern "C" long long psld_conv3x3_wino_frag_bytes(int cout, int cin) { return (long long)cout * cin * 16 * 6 + 16384; }
// two limbs (PSLD_MATH_BF16X3): 2/3 of the payload, the same pad
extern "C" long long psld_conv3x3_wino_frag_bytes_x3(int cout, int cin) { return (long long)cout * cin * 16 * 4 + 16384; }

// one fp16 plane (eval math f16): 1/3 of the payload, the same pad
extern "C" long long psld_conv3x3_wino_frag_bytes_f16(int cout, int cin) { return (long long)cout * cin * 16 * 2 + 16384; }

// cout: a multiple of 128, or of 32 from 128 up (the last channel tile cut short: wino_conv8s_kernel<..., TAIL = true>)
extern "C" int psld_conv3x3_wino_supported(int c1, int c2, int batch, int h, int w, int cout) {
    int nseg, rps, halo;
    return c1 > 0 && c2 >= 0 && c1 % 32 == 0 && c2 % 32 == 0 && cout >= 128 && cout % 32 == 0 && batch > 0 &&
           wino_geometry(h, w, &nseg, &rps, &halo);
}

extern "C" int psld_pack_conv3x3_wino(const float* w_oihw, void* ufrag, int cout, int cin, int dgrad, hipStream_t stream) {
    PSLD_CHECK_ARG(w_oihw && ufrag && aligned16(ufrag), "psld_pack_conv3x3_wino: null / unaligned pointer");
    const int n_out = dgrad ? cin : cout, k_in = dgrad ? cout : cin;
    PSLD_CHECK_ARG(n_out >= 128 && k_in > 0 && n_out % 32 == 0 && k_in % 32 == 0,
                   "psld_pack_conv3x3_wino: needs out channels %%32 (>= 128) and in channels %%32 (got %d, %d)", n_out, k_in);
    const long long items = (long long)(n_out / 16) * (k_in / 32) * 64;
    const unsigned blocks = psld_grid_blocks(items, 64, 16384);
    if (dgrad) hipLaunchKernelGGL(wino_pack_kernel<3>, dim3(blocks), dim3(64), 0, stream, w_oihw, reinterpret_cast<u32x4*>(ufrag),
                                  n_out, k_in, 9LL, (long long)cin * 9, 1);
    else hipLaunchKernelGGL(wino_pack_kernel<3>, dim3(blocks), dim3(64), 0, stream, w_oihw, reinterpret_cast<u32x4*>(ufrag),
                            n_out, k_in, (long long)cin * 9, 9LL, 0);
    PSLD_CHECK_LAUNCH("psld_pack_conv3x3_wino");
    return PSLD_OK;
}

extern "C" int psld_pack_conv3x3_wino_x3(const float* w_oihw, void* ufrag, int cout, int cin, hipStream_t stream) {
    PSLD_CHECK_ARG(w_oihw && ufrag && aligned16(ufrag), "psld_pack_conv3x3_wino_x3: null / unaligned pointer");
    PSLD_CHECK_ARG(cout >= 128 && cin > 0 && cout % 32 == 0 && cin % 32 == 0,
                   "psld_pack_conv3x3_wino_x3: needs out channels %%32 (>= 128) and in channels %%32 (got %d, %d)", cout, cin);
    const long long items = (long long)(cout / 16) * (cin / 32) * 64;
    const unsigned blocks = psld_grid_blocks(items, 64, 16384);
    hipLaunchKernelGGL(wino_pack_kernel<2>, dim3(blocks), dim3(64), 0, stream, w_oihw, reinterpret_cast<u32x4*>(ufrag), cout, cin,
                       (long long)cin * 9, 9LL, 0);
    PSLD_CHECK_LAUNCH("psld_pack_conv3x3_wino_x3");
    return PSLD_OK;
}

extern "C" int psld_pack_conv3x3_wino_f16(const float* w_oihw, void* ufrag, int cout, int cin, hipStream_t stream) {
    PSLD_CHECK_ARG(w_oihw && ufrag && aligned16(ufrag), "psld_pack_conv3x3_wino_f16: null / unaligned pointer");
    PSLD_CHECK_ARG(cout >= 128 && cin > 0 && cout % 32 == 0 && cin % 32 == 0,
                   "psld_pack_conv3x3_wino_f16: needs out channels %%32 (>= 128) and in channels %%32 (got %d, %d)", cout, cin);
    const long long items = (long long)(cout / 16) * (cin / 32) * 64;
    const unsigned blocks = psld_grid_blocks(items, 64, 16384);
    hipLaunchKernelGGL(wino_pack_kernel<1>, dim3(blocks), dim3(64), 0, stream, w_oihw, reinterpret_cast<u32x4*>(ufrag), cout, cin,
                       (long long)cin * 9, 9LL, 0);
    PSLD_CHECK_LAUNCH("psld_pack_conv3x3_wino_f16");
    return PSLD_OK;
}

// the data-gradient orientation as one fp16 plane (record f16): the transposed, rotated weights, U rounded once
extern "C" int psld_pack_conv3x3_wino_dgrad_f16(const float* w_oihw, void* ufrag, int cout, int cin, hipStream_t stream) {
    PSLD_CHECK_ARG(w_oihw && ufrag && aligned16(ufrag), "psld_pack_conv3x3_wino_dgrad_f16: null / unaligned pointer");
    PSLD_CHECK_ARG(cin >= 128 && cout > 0 && cin % 32 == 0 && cout % 32 == 0,
                   "psld_pack_conv3x3_wino_dgrad_f16: needs in channels %%32 (>= 128) and out channels %%32 (got %d, %d)", cin, cout);
    const long long items = (long long)(cin / 16) * (cout / 32) * 64;
    hipLaunchKernelGGL(wino_pack_kernel<1>, dim3(psld_grid_blocks(items, 64, 16384)), dim3(64), 0, stream, w_oihw,
                       reinterpret_cast<u32x4*>(ufrag), cin, cout, 9LL, (long long)cin * 9, 1);
    PSLD_CHECK_LAUNCH("psld_pack_conv3x3_wino_dgrad_f16");
    return PSLD_OK;
}

// the data-gradient orientation on two limbs (record math PSLD_MATH_BF16X3): psld_pack_conv3x3_wino(..., dgrad = 1)'s planes 0 and 1
extern "C" int psld_pack_conv3x3_wino_dgrad_x3(const float* w_oihw, void* ufrag, int cout, int cin, hipStream_t stream) {
    PSLD_CHECK_ARG(w_oihw && ufrag && aligned16(ufrag), "psld_pack_conv3x3_wino_dgrad_x3: null / unaligned pointer");
    PSLD_CHECK_ARG(cin >= 128 && cout > 0 && cin % 32 == 0 && cout % 32 == 0,
                   "psld_pack_conv3x3_wino_dgrad_x3: needs in channels %%32 (>= 128) and out channels %%32 (got %d, %d)", cin, cout);
    const long long items = (long long)(cin / 16) * (cout / 32) * 64;
    hipLaunchKernelGGL(wino_pack_kernel<2>, dim3(psld_grid_blocks(items, 64, 16384)), dim3(64), 0, stream, w_oihw,
                       reinterpret_cast<u32x4*>(ufrag), cin, cout, 9LL, (long long)cin * 9, 1);
    PSLD_CHECK_LAUNCH("psld_pack_conv3x3_wino_dgrad_x3");
    return PSLD_OK;
}

extern "C" int psld_pack_wino_batch_x3(const long long* table_dev, int entries, long long total_items, hipStream_t stream) {
    PSLD_CHECK_ARG(table_dev && entries > 0 && total_items > 0, "psld_pack_wino_batch_x3: bad args");
    hipLaunchKernelGGL(wino_pack_batch_kernel<2>, dim3(psld_grid_blocks(total_items, 64, 32768)), dim3(64), 0, stream,
                       table_dev, entries, total_items);
    PSLD_CHECK_LAUNCH("psld_pack_wino_batch_x3");
    return PSLD_OK;
}

extern "C" int psld_pack_wino_batch_f16(const long long* table_dev, int entries, long long total_items, hipStream_t stream) {
    PSLD_CHECK_ARG(table_dev && entries > 0 && total_items > 0, "psld_pack_wino_batch_f16: bad args");
    hipLaunchKernelGGL(wino_pack_batch_kernel<1>, dim3(psld_grid_blocks(total_items, 64, 32768)), dim3(64), 0, stream,
                       table_dev, entries, total_items);
    PSLD_CHECK_LAUNCH("psld_pack_wino_batch_f16");
    return PSLD_OK;
}

extern "C" int psld_pack_wino_batch(const long long* table_dev, int entries, long long total_items, hipStream_t stream) {
    PSLD_CHECK_ARG(table_dev && entries > 0 && total_items > 0, "psld_pack_wino_batch: bad args");
    hipLaunchKernelGGL(wino_pack_batch_kernel<3>, dim3(psld_grid_blocks(total_items, 64, 32768)), dim3(64), 0, stream,
                       table_dev, entries, total_items);
    PSLD_CHECK_LAUNCH("psld_pack_wino_batch");
    return PSLD_OK;
}

#ifdef PSLD_ABLATIONS
static unsigned long long* g_wino_dbg = nullptr;
// ablation library only: device buffer for the s_memtime stamps of PSLD_WINO_ABL=64 ([workgroups][8 waves][8] uint64)
extern "C" void psld_abl_set_wino_debug(unsigned long long* p) { g_wino_dbg = p; }
#endif

namespace {
struct WinoGn {
    const float *sc1, *sh1, *sc2, *sh2;
    int act;
};
int wino_conv(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w, const void* ufrag, int cout, float* y,
              int ldy, const psld_epilogue_t* epi, const WinoGn* gn, void* workspace, long long ws_bytes, hipStream_t stream,
              int nl = 3, int shift = -1);
}  // namespace

extern "C" int psld_conv3x3_wino_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                                     const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                     hipStream_t stream) {
    return wino_conv(x1, c1, x2, c2, batch, h, w, ufrag, cout, y, ldy, epi, nullptr, nullptr, 0, stream);
}

// K splits a launch of this shape takes when it is given a workspace (1: none) and the bytes that workspace needs
extern "C" int psld_conv3x3_wino_ksplit(int c1, int c2, int batch, int h, int w, int cout) {
    if (!psld_conv3x3_wino_supported(c1, c2, batch, h, w, cout)) return 1;
    int nseg, rps, halo;
    wino_geometry(h, w, &nseg, &rps, &halo);
    const int tiles = wino_tiles_m(batch, h, w, nseg) * cdiv(cout, 128), chunks = (c1 + c2) / 32;
    const int cus = wino_cu_count();
    int ks = 1;
    // one workgroup per CU: a grid below half a round leaves CUs idle - split the channel chunks so that it fills one round
    while (tiles * ks * 2 <= cus && chunks % (ks * 2) == 0 && chunks / (ks * 2) >= 2) ks *= 2;
    return ks;
}
extern "C" long long psld_conv3x3_wino_ws_bytes(int c1, int c2, int batch, int h, int w, int cout) {
    const int ks = psld_conv3x3_wino_ksplit(c1, c2, batch, h, w, cout);
    return ks > 1 ? (long long)ks * batch * h * w * cout * 4 : 0;
}

extern "C" int psld_conv3x3_wino_ws_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                                        const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                        void* workspace, long long ws_bytes, hipStream_t stream) {
    return wino_conv(x1, c1, x2, c2, batch, h, w, ufrag, cout, y, ldy, epi, nullptr, workspace, ws_bytes, stream);
}

extern "C" int psld_conv3x3_wino_gn_supported(int c1, int c2, int batch, int h, int w, int cout) {
    // one image per workgroup region; whole 128-channel tiles (no channel tail in the GroupNorm-fused staging)
    return psld_conv3x3_wino_supported(c1, c2, batch, h, w, cout) && h * w >= 128 && cout % 128 == 0;
}

extern "C" int psld_conv3x3_wino_gn_f32(const float* x1, int c1, const float* scale1, const float* shift1, const float* x2,
                                        int c2, const float* scale2, const float* shift2, int act, int batch, int h, int w,
                                        const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                        hipStream_t stream) {
    PSLD_CHECK_ARG(scale1 && shift1 && (c2 == 0 || (scale2 && shift2)), "psld_conv3x3_wino_gn_f32: null scale / shift");
    PSLD_CHECK_ARG(psld_conv3x3_wino_gn_supported(c1, c2, batch, h, w, cout),
                   "psld_conv3x3_wino_gn_f32: unsupported shape c1=%d c2=%d %dx%d cout=%d (needs h*w >= 128)", c1, c2, h, w, cout);
    PSLD_CHECK_ARG(aligned16(scale1) && aligned16(shift1) && (c2 == 0 || (aligned16(scale2) && aligned16(shift2))),
                   "psld_conv3x3_wino_gn_f32: unaligned scale / shift");
    const WinoGn gn{scale1, shift1, scale2, shift2, act};
    return wino_conv(x1, c1, x2, c2, batch, h, w, ufrag, cout, y, ldy, epi, &gn, nullptr, 0, stream);
}

extern "C" int psld_conv3x3_wino_gn_ws_f32(const float* x1, int c1, const float* scale1, const float* shift1, const float* x2,
                                           int c2, const float* scale2, const float* shift2, int act, int batch, int h, int w,
                                           const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                           void* workspace, long long ws_bytes, hipStream_t stream) {
    PSLD_CHECK_ARG(scale1 && shift1 && (c2 == 0 || (scale2 && shift2)), "psld_conv3x3_wino_gn_ws_f32: null scale / shift");
    PSLD_CHECK_ARG(psld_conv3x3_wino_gn_supported(c1, c2, batch, h, w, cout),
                   "psld_conv3x3_wino_gn_ws_f32: unsupported shape c1=%d c2=%d %dx%d cout=%d (needs h*w >= 128)", c1, c2, h, w, cout);
    PSLD_CHECK_ARG(aligned16(scale1) && aligned16(shift1) && (c2 == 0 || (aligned16(scale2) && aligned16(shift2))),
                   "psld_conv3x3_wino_gn_ws_f32: unaligned scale / shift");
    const WinoGn gn{scale1, shift1, scale2, shift2, act};
    return wino_conv(x1, c1, x2, c2, batch, h, w, ufrag, cout, y, ldy, epi, &gn, workspace, ws_bytes, stream);
}

// ---- two limbs (PSLD_MATH_BF16X3): the forward launches above on fragments of psld_pack_conv3x3_wino_x3 ----------------------
extern "C" int psld_conv3x3_wino_x3_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                                        const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                        void* workspace, long long ws_bytes, hipStream_t stream) {
    return wino_conv(x1, c1, x2, c2, batch, h, w, ufrag, cout, y, ldy, epi, nullptr, workspace, ws_bytes, stream, 2);
}

extern "C" int psld_conv3x3_wino_gn_x3_f32(const float* x1, int c1, const float* scale1, const float* shift1, const float* x2,
                                           int c2, const float* scale2, const float* shift2, int act, int batch, int h, int w,
                                           const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                           void* workspace, long long ws_bytes, hipStream_t stream) {
    PSLD_CHECK_ARG(scale1 && shift1 && (c2 == 0 || (scale2 && shift2)), "psld_conv3x3_wino_gn_x3_f32: null scale / shift");
    PSLD_CHECK_ARG(psld_conv3x3_wino_gn_supported(c1, c2, batch, h, w, cout),
                   "psld_conv3x3_wino_gn_x3_f32: unsupported shape c1=%d c2=%d %dx%d cout=%d (needs h*w >= 128)", c1, c2, h, w, cout);
    PSLD_CHECK_ARG(aligned16(scale1) && aligned16(shift1) && (c2 == 0 || (aligned16(scale2) && aligned16(shift2))),
                   "psld_conv3x3_wino_gn_x3_f32: unaligned scale / shift");
    const WinoGn gn{scale1, shift1, scale2, shift2, act};
    return wino_conv(x1, c1, x2, c2, batch, h, w, ufrag, cout, y, ldy, epi, &gn, workspace, ws_bytes, stream, 2);
}

// ---- one fp16 plane (eval math f16): the same launches on fragments of psld_pack_conv3x3_wino_f16 ----------------------------
extern "C" int psld_conv3x3_wino_f16_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                                         const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                         void* workspace, long long ws_bytes, hipStream_t stream) {
    return wino_conv(x1, c1, x2, c2, batch, h, w, ufrag, cout, y, ldy, epi, nullptr, workspace, ws_bytes, stream, 1);
}

extern "C" int psld_conv3x3_wino_gn_f16_f32(const float* x1, int c1, const float* scale1, const float* shift1, const float* x2,
                                            int c2, const float* scale2, const float* shift2, int act, int batch, int h, int w,
                                            const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi,
                                            void* workspace, long long ws_bytes, hipStream_t stream) {
    PSLD_CHECK_ARG(scale1 && shift1 && (c2 == 0 || (scale2 && shift2)), "psld_conv3x3_wino_gn_f16_f32: null scale / shift");
    PSLD_CHECK_ARG(psld_conv3x3_wino_gn_supported(c1, c2, batch, h, w, cout),
                   "psld_conv3x3_wino_gn_f16_f32: unsupported shape c1=%d c2=%d %dx%d cout=%d (needs h*w >= 128)", c1, c2, h, w, cout);
    PSLD_CHECK_ARG(aligned16(scale1) && aligned16(shift1) && (c2 == 0 || (aligned16(scale2) && aligned16(shift2))),
                   "psld_conv3x3_wino_gn_f16_f32: unaligned scale / shift");
    const WinoGn gn{scale1, shift1, scale2, shift2, act};
    return wino_conv(x1, c1, x2, c2, batch, h, w, ufrag, cout, y, ldy, epi, &gn, workspace, ws_bytes, stream, 1);
}

// ---- the same with an operand shift (record f16: data gradients): x1 | x2 times 2^shift before the rounding, 2^-shift in alpha ----
extern "C" int psld_conv3x3_wino_f16s_f32(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w,
                                          const void* ufrag, int cout, float* y, int ldy, const psld_epilogue_t* epi, int shift,
                                          void* workspace, long long ws_bytes, hipStream_t stream) {
    PSLD_CHECK_ARG(shift >= 0 && shift <= 24, "psld_conv3x3_wino_f16s_f32: shift %d outside 0..24", shift);
    return wino_conv(x1, c1, x2, c2, batch, h, w, ufrag, cout, y, ldy, epi, nullptr, workspace, ws_bytes, stream, 1, shift);
}

namespace {
// LA = 3: a position is two MFMAs here (six on two limbs), so the fragments are requested one position further ahead
int wino_launch_f16(const WinoArgs& a, bool gn, hipStream_t stream) {
    if (gn) return launch_wino8s<0, true, false, 3, false, 1>(a, stream, "psld_conv3x3_wino_gn_f16_f32");
    if (a.N % 128) return launch_wino8s<0, false, false, 3, true, 1>(a, stream, "psld_conv3x3_wino_f16_f32");
    return launch_wino8s<0, false, false, 3, false, 1>(a, stream, "psld_conv3x3_wino_f16_f32");
}

// operand shift (no GroupNorm-fused form: a recording pass has none)
int wino_launch_f16s(const WinoArgs& a, hipStream_t stream) {
    if (a.N % 128) return launch_wino8s<0, false, false, 3, true, 1, true>(a, stream, "psld_conv3x3_wino_f16s_f32");
    return launch_wino8s<0, false, false, 3, false, 1, true>(a, stream, "psld_conv3x3_wino_f16s_f32");
}

int wino_launch_x3(const WinoArgs& a, bool gn, hipStream_t stream) {
    if (gn) return launch_wino8s<0, true, false, 2, false, 2>(a, stream, "psld_conv3x3_wino_gn_x3_f32");
    if (a.N % 128) return launch_wino8s<0, false, false, 2, true, 2>(a, stream, "psld_conv3x3_wino_x3_f32");
    return launch_wino8s<0, false, false, 2, false, 2>(a, stream, "psld_conv3x3_wino_x3_f32");
}

int wino_conv(const float* x1, int c1, const float* x2, int c2, int batch, int h, int w, const void* ufrag, int cout, float* y,
              int ldy, const psld_epilogue_t* epi, const WinoGn* gn, void* workspace, long long ws_bytes, hipStream_t stream,
              int nl, int shift) {
    PSLD_CHECK_ARG(x1 && ufrag && y && (c2 == 0 || x2), "psld_conv3x3_wino_f32: null pointer");
    PSLD_CHECK_ARG(psld_conv3x3_wino_supported(c1, c2, batch, h, w, cout),
                   "psld_conv3x3_wino_f32: unsupported shape c1=%d c2=%d %dx%d cout=%d", c1, c2, h, w, cout);
    PSLD_CHECK_ARG(aligned16(x1) && (!x2 || aligned16(x2)) && aligned16(ufrag), "psld_conv3x3_wino_f32: unaligned pointer");
    WinoArgs a{};
    a.x1 = x1; a.x2 = x2; a.C1 = c1; a.C2 = c2;
    a.B = batch; a.H = h; a.W = w;
    a.ufrag = reinterpret_cast<const u32x4*>(ufrag);
    a.N = cout; a.M = batch * h * w;
    a.chunks = (c1 + c2) / 32;
    a.C = y; a.ldc = ldy;
    int halo_px = 0;
    wino_geometry(h, w, &a.nseg, &a.rps, &halo_px);
    a.e = make_epilogue(epi);
    if (shift >= 0) {       // psld_conv3x3_wino_f16s_f32: both factors are powers of two - the rounding to fp16 is the only error
        a.opscale = ldexpf(1.f, shift);
        a.e.alpha *= ldexpf(1.f, -shift);       // the split-chunk form applies e in its reduction pass: covered as well
    }
    const PsldEpilogue& e = a.e;
    PSLD_CHECK_ARG(!e.gn_part || (e.gn_hw == h * w && e.gn_hw % 64 == 0 && !e.accumulate && cout % 128 == 0),
                   "psld_conv3x3_wino_f32: gn_part needs gn_hw = h*w, a multiple of 64, no accumulation and cout %% 128 == 0");
    PSLD_CHECK_ARG(ldy % 4 == 0 && aligned16(y) && (!e.res || (e.ldres % 4 == 0 && aligned16(e.res))) &&
                       (!e.bias || aligned16(e.bias)) && (!e.rowbias || (e.ld_rowbias % 4 == 0 && aligned16(e.rowbias))),
                   "limb kernels: y, residual, bias and rowbias need 16-byte aligned rows (pointer and row stride)");
    // the epilogue addresses a region's operands by 32-bit byte offsets from its first pixel: below 512 pixels x row stride
    PSLD_CHECK_ARG(ldy > 0 && ldy < (1 << 20) && (!e.res || (e.ldres > 0 && e.ldres < (1 << 20))),
                   "psld_conv3x3_wino_*: row strides of y and the residual must be below 2^20 elements");
    a.zero = psld_detail_zero_page("psld_conv3x3_wino_f32");
    if (!a.zero) return PSLD_ERR_LAUNCH;
    a.nmajor = 1;       // channel-tile-major: an XCD streams ONE 128-channel slice of U at a time (pixel-tile-major measured 1-2 % slower)
    const char* name = "psld_conv3x3_wino_f32";
    a.cw = w;
    if (w >= 64) {      // 4 x 32 pixel blocks: the 32x32 level's halo (6 x 34 = 204 pixels); W / 32 blocks per row band
        a.cw = 32; a.rps = 4; a.nseg = 1;
        halo_px = 6 * 34;
    }
    // the kernel's divisors (WinoArgs): every one a power of two or on the proven multiply-shift list
    a.tiles_m = wino_tiles_m(batch, h, w, a.nseg);
    a.lg_tiles_x = wino_lg2(a.cw >> 1);
    a.lg_tps = wino_lg2((a.rps >> 1) * (a.cw >> 1));
    a.lg_xblocks = wino_lg2(w / a.cw);
    a.lg_rpi = h * w >= 128 ? wino_lg2((h * w) >> 7) : 0;
    a.lg_ksplit = 0;
    a.mul_seg = wino_mul16((a.rps + 2) * (a.cw + 2));
    a.mul_w2 = wino_mul16(a.cw + 2);
    a.rb_img = e.rowbias && e.rows_per_img == h * w;
    PSLD_CHECK_ARG(wino_geo_listed(a.rps, a.cw) && a.lg_tiles_x >= 0 && a.lg_tps >= 0 && a.lg_xblocks >= 0,
                   "psld_conv3x3_wino_*: no divisor table for the geometry of %dx%d", h, w);
    if (gn) {
        a.gsc1 = gn->sc1; a.gsh1 = gn->sh1; a.gsc2 = gn->sc2; a.gsh2 = gn->sh2; a.gn_act = gn->act;
    }
    // Small grids (the 8x8 level at training batches: 128 workgroups for 256 CUs): split the channel chunks over ksplit
    // workgroups per tile, plain partial outputs into the workspace, summed + the whole epilogue by conv_reduce_epilogue -
    // what the direct kernels do for the same shapes (GroupNorm partial sums of the output: formed by that pass).  The GroupNorm-
    // fused form splits the same way (same chunk ranges, same reduction: bitwise the unfused pair).
    const int ks = workspace ? psld_conv3x3_wino_ksplit(c1, c2, batch, h, w, cout) : 1;
    if (ks > 1 && (!e.gn_part || psld_detail_conv_reduce_gn_ok(a.M, cout, e)) && ws_bytes >= (long long)ks * a.M * cout * 4 && aligned16(workspace)) {
        WinoArgs s = a;
        s.ksplit = ks;
        s.lg_ksplit = wino_lg2(ks);        // a power of two (psld_conv3x3_wino_ksplit)
        s.rb_img = 0;
        s.slab_stride = (long long)a.M * cout;
        s.C = reinterpret_cast<float*>(workspace);
        s.ldc = cout;
        s.e = make_epilogue(nullptr);
        const int rc = shift >= 0 ? wino_launch_f16s(s, stream)
                       : nl == 1 ? wino_launch_f16(s, gn != nullptr, stream)
                       : nl == 2 ? wino_launch_x3(s, gn != nullptr, stream)
                       : gn    ? launch_wino8s<0, true>(s, stream, "psld_conv3x3_wino_gn_f32")
                               : (cout % 128 ? launch_wino8s<0, false, false, 2, true>(s, stream, name) : launch_wino8s<0>(s, stream, name));
        if (rc != PSLD_OK) return rc;
        return psld_detail_conv_reduce_epilogue(s.C, ks, a.M, cout, y, ldy, e, stream);
    }
    if (shift >= 0) return wino_launch_f16s(a, stream);
    if (nl == 1) return wino_launch_f16(a, gn != nullptr, stream);
    if (nl == 2) return wino_launch_x3(a, gn != nullptr, stream);
    if (gn) return launch_wino8s<0, true>(a, stream, "psld_conv3x3_wino_gn_f32");
    if (cout % 128) return launch_wino8s<0, false, false, 2, true>(a, stream, name);      // last channel tile cut short
#ifdef PSLD_ABLATIONS      // libpsld_hip_abl.so only: the variants of conv_wino_abl.inc and the timing-only ablations (wrong results)
#include "conv_wino_abl_dispatch.inc"
#endif
    return launch_wino8s<0>(a, stream, name);
}
}  // namespace
