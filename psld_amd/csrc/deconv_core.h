// The per-plane arithmetic of the deconv kernels (deconv.hip; DESIGN section 13, "Deconvolution"): the 2-D DFT of ONE real H x W plane held
// in LDS, the work of one workgroup.  H and W are powers of two, H >= 2, W >= 4.
//
//   packing:   z[r][j] = x[r][2j] + i x[r][2j+1], an H x M complex array, M = W / 2 (half the storage of the plane as complex
//              numbers: 128 x 64 x 16 B = 128 KiB at 128 x 128), rows P = M + 1 elements apart (no two rows of a column on
//              one LDS bank group);
//   forward:   decimation in frequency along the rows, then along the columns - natural order in, bit-reversed order out, so
//              Z[k1][k2] lies at z[rev_H(k1)][rev_M(k2)] and no permutation pass is needed;
//   spectrum:  X[k1][k2] = E + w^k2 O, E = (A + B) / 2, O = (A - B) / 2i, A = Z[k1][k2 mod M], B = conj Z[-k1][-k2 mod M],
//              w = exp(-2 pi i / W), for the Hermitian half k2 = 0 .. M.  The two entries {Z[k1][k2], Z[-k1][-k2]} give
//              X[k1][k2] and X[-k1][M - k2] (and, for k2 = 0, also X[-k1][0] and X[k1][M]); after the pointwise filter G = F(X)
//              the same two G give back Zg[k1][k2] = (G[k1][k2] + conj G[-k1][M-k2]) / 2 + i w^-k2 (G[k1][k2] - conj G[-k1][M-k2]) / 2
//              and Zg[-k1][-k2]: ONE thread owns the pair in registers, so the filter runs in place without a barrier;
//   inverse:   decimation in time along the columns, then the rows - bit-reversed in, natural out, unscaled (the caller
//              divides by H M): g[r][2j] + i g[r][2j+1].
//
// float64 throughout.  Every loop is a strided loop over the items of one phase followed by a barrier, so the same text
// compiles for the host with one "thread" (tid 0 of 1) and no barrier: that is how the arithmetic is tested without a GPU.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_HD __host__ __device__ __forceinline__
#else
#define DC_HD inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define DC_SYNC() __syncthreads()
#else
#define DC_SYNC() ((void)0)
#endif
#define DC_FOR(i, n) for (int i = tid; i < (n); i += nthr)

struct alignas(16) dc2 {
    double x, y;
};
DC_HD dc2 dc_make(double x, double y) { dc2 r; r.x = x; r.y = y; return r; }
DC_HD dc2 dc_add(dc2 a, dc2 b) { return dc_make(a.x + b.x, a.y + b.y); }
DC_HD dc2 dc_sub(dc2 a, dc2 b) { return dc_make(a.x - b.x, a.y - b.y); }
DC_HD dc2 dc_mul(dc2 a, dc2 b) { return dc_make(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
DC_HD dc2 dc_conj(dc2 a) { return dc_make(a.x, -a.y); }
DC_HD dc2 dc_scale(dc2 a, double s) { return dc_make(a.x * s, a.y * s); }
DC_HD dc2 dc_times_i(dc2 a) { return dc_make(-a.y, a.x); }
DC_HD dc2 dc_over_i(dc2 a) { return dc_make(a.y, -a.x); }

DC_HD int dc_rev(int k, int lg) { return (int)(__builtin_bitreverse32((unsigned)k) >> (32 - lg)); }

// geometry of one plane; tw[k] = exp(-2 pi i k / n), k < n / 2, n = max(H, W)
struct dc_geom {
    int h, m, lgh, lgm, p, n;  // m = W / 2, p = m + 1 the row pitch
};
DC_HD dc_geom dc_geometry(int h, int w, int lgh, int lgw) {
    dc_geom g;
    g.h = h; g.m = w / 2; g.lgh = lgh; g.lgm = lgw - 1; g.p = g.m + 1; g.n = h > w ? h : w;
    return g;
}
// elements of LDS: the plane, then the twiddles
DC_HD int dc_plane_elems(const dc_geom& g) { return g.h * g.p; }
DC_HD int dc_lds_elems(const dc_geom& g) { return g.h * g.p + g.n / 2; }

// ---- butterflies ----------------------------------------------------------------------------------------------------------
// one level of every row transform: half-span hs, element stride 1; FWD: (a + b, (a - b) t), else (a + t~ b, a - t~ b)
template <bool FWD>
DC_HD void dc_level_rows(dc2* z, const dc2* tw, const dc_geom& g, int hs, int lghs, int tid, int nthr) {
    const int half = g.m >> 1, lghalf = g.lgm - 1, tstep = g.n >> (lghs + 1);
    DC_FOR(j, g.h * half) {
        const int r = j >> lghalf, b = j & (half - 1);
        const int pos = b & (hs - 1), i0 = r * g.p + ((b >> lghs) << (lghs + 1)) + pos, i1 = i0 + hs;
        dc2 t = tw[pos * tstep];
        const dc2 a = z[i0], c = z[i1];
        if (FWD) {
            z[i0] = dc_add(a, c);
            z[i1] = dc_mul(dc_sub(a, c), t);
        } else {
            const dc2 d = dc_mul(c, dc_conj(t));
            z[i0] = dc_add(a, d);
            z[i1] = dc_sub(a, d);
        }
    }
    DC_SYNC();
}
// ... of every column transform: element stride p
template <bool FWD>
DC_HD void dc_level_cols(dc2* z, const dc2* tw, const dc_geom& g, int hs, int lghs, int tid, int nthr) {
    const int half = g.h >> 1, tstep = g.n >> (lghs + 1);
    DC_FOR(j, half * g.m) {
        const int col = j & (g.m - 1), b = j >> g.lgm;
        const int pos = b & (hs - 1), i0 = (((b >> lghs) << (lghs + 1)) + pos) * g.p + col, i1 = i0 + hs * g.p;
        dc2 t = tw[pos * tstep];
        const dc2 a = z[i0], c = z[i1];
        if (FWD) {
            z[i0] = dc_add(a, c);
            z[i1] = dc_mul(dc_sub(a, c), t);
        } else {
            const dc2 d = dc_mul(c, dc_conj(t));
            z[i0] = dc_add(a, d);
            z[i1] = dc_sub(a, d);
        }
    }
    DC_SYNC();
}

// natural order in, Z[k1][k2] at z[rev(k1) p + rev(k2)] out; the caller has synchronised after filling z and tw
DC_HD void dc_forward(dc2* z, const dc2* tw, const dc_geom& g, int tid, int nthr) {
    for (int lg = g.lgm - 1; lg >= 0; --lg) dc_level_rows<true>(z, tw, g, 1 << lg, lg, tid, nthr);
    for (int lg = g.lgh - 1; lg >= 0; --lg) dc_level_cols<true>(z, tw, g, 1 << lg, lg, tid, nthr);
}
// the inverse of dc_forward times H M
DC_HD void dc_inverse(dc2* z, const dc2* tw, const dc_geom& g, int tid, int nthr) {
    for (int lg = 0; lg < g.lgh; ++lg) dc_level_cols<false>(z, tw, g, 1 << lg, lg, tid, nthr);
    for (int lg = 0; lg < g.lgm; ++lg) dc_level_rows<false>(z, tw, g, 1 << lg, lg, tid, nthr);
}

DC_HD void dc_twiddles(dc2* tw, const dc_geom& g, int tid, int nthr) {
    DC_FOR(k, g.n / 2) {
        const double x = 2.0 * (double)k / (double)g.n;  // exact: n is a power of two
        double s, c;
#if defined(__HIP_DEVICE_COMPILE__)
        sincospi(x, &s, &c);
#else
        s = sin(3.14159265358979323846 * x);
        c = cos(3.14159265358979323846 * x);
#endif
        tw[k] = dc_make(c, -s);
    }
}

// w^k, w = exp(-2 pi i / W), k = 0 .. M
DC_HD dc2 dc_tw_w(const dc2* tw, const dc_geom& g, int k) {
    return k == g.m ? dc_make(-1.0, 0.0) : tw[k * (g.n / (2 * g.m))];
}

// X[k1][k2] of the real plane from A = Z[k1][k2 mod M], Bc = Z[-k1][-k2 mod M] (not yet conjugated), t = w^k2
DC_HD dc2 dc_untangle(dc2 a, dc2 bc, dc2 t) {
    const dc2 b = dc_conj(bc);
    const dc2 e = dc_scale(dc_add(a, b), 0.5), o = dc_over_i(dc_scale(dc_sub(a, b), 0.5));
    return dc_add(e, dc_mul(t, o));
}
// Zg[k1][k2] from G[k1][k2], Gr = G[-k1][M - k2] and t = w^k2
DC_HD dc2 dc_tangle(dc2 ga, dc2 gr, dc2 t) {
    const dc2 c = dc_conj(gr);
    const dc2 e = dc_scale(dc_add(ga, c), 0.5), o = dc_mul(dc_conj(t), dc_scale(dc_sub(ga, c), 0.5));
    return dc_add(e, dc_times_i(o));
}

// ---- the pointwise filters: G = F(X) at (k1, k2) of the half spectrum, index k1 (M + 1) + k2 of hhat / yhat ---------------------
// g^ = conj(h^) (s2 + r2) / (s2 + r2 |h^|^2) (y^ - h^ x^); a frequency with denominator 0 measures nothing: 0
struct dc_measure_filter {
    const dc2* hhat;
    const dc2* yhat;
    double s2, r2;
    DC_HD dc2 operator()(int idx, dc2 x) const {
        const dc2 hh = hhat[idx];
        const double den = s2 + r2 * (hh.x * hh.x + hh.y * hh.y);
        if (den == 0.0) return dc_make(0.0, 0.0);
        const dc2 res = dc_sub(yhat[idx], dc_mul(hh, x));
        return dc_mul(dc_scale(dc_conj(hh), (s2 + r2) / den), res);
    }
};
// A x (adjoint: A^T x)
struct dc_apply_filter {
    const dc2* hhat;
    bool adjoint;
    DC_HD dc2 operator()(int idx, dc2 x) const {
        const dc2 hh = hhat[idx];
        return dc_mul(adjoint ? dc_conj(hh) : hh, x);
    }
};

// in place on the output of dc_forward: z becomes the input of dc_inverse for the plane with spectrum F(X).  WRITE: instead,
// leave z alone and store X itself to spec (the half spectrum, [H][M + 1]).
template <bool WRITE, class F>
DC_HD void dc_filter(dc2* z, const dc2* tw, const dc_geom& g, const F& f, dc2* spec, int tid, int nthr) {
    const int mp = g.m + 1;
    DC_FOR(i, g.h * g.m) {
        const int k1 = i >> g.lgm, k2 = i & (g.m - 1);
        const int q1 = (g.h - k1) & (g.h - 1), q2 = (g.m - k2) & (g.m - 1);
        if (q1 * g.m + q2 < i) continue;  // the partner's thread owns the pair
        const bool self = q1 == k1 && q2 == k2;
        const int ip = dc_rev(k1, g.lgh) * g.p + dc_rev(k2, g.lgm), iq = dc_rev(q1, g.lgh) * g.p + dc_rev(q2, g.lgm);
        const dc2 zp = z[ip], zq = z[iq];
        const dc2 ta = dc_tw_w(tw, g, k2), tb = dc_tw_w(tw, g, g.m - k2);
        // a = (k1, k2), b = (-k1, M - k2)
        const int ia = k1 * mp + k2, ib = q1 * mp + (g.m - k2);
        const dc2 xa = dc_untangle(zp, zq, ta), xb = dc_untangle(zq, zp, tb);
        if (WRITE) {
            spec[ia] = xa;
            spec[ib] = xb;
        } else {
            const dc2 ga = f(ia, xa), gb = f(ib, xb);
            z[ip] = dc_tangle(ga, gb, ta);
            if (!self && k2 != 0) z[iq] = dc_tangle(gb, ga, tb);
        }
        if (k2 == 0 && !self) {
            // c = (-k1, 0), d = (k1, M): the other two entries of the half spectrum that this pair holds
            const dc2 one = dc_make(1.0, 0.0), minus = dc_make(-1.0, 0.0);
            const int ic = q1 * mp, id = k1 * mp + g.m;
            const dc2 xc = dc_untangle(zq, zp, one), xd = dc_untangle(zp, zq, minus);
            if (WRITE) {
                spec[ic] = xc;
                spec[id] = xd;
            } else {
                z[iq] = dc_tangle(f(ic, xc), f(id, xd), one);
            }
        }
    }
    DC_SYNC();
}

// ---- super-resolution: A = D_s C_k, a periodic blur followed by keeping every s-th sample ("Super-resolution") ---
// A A^T is circulant on the H/s x W/s grid with eigenvalues Lambda, so the measure step is three transform pairs on ONE
// plane storage: z = k (*) x0^ at full size, rho = y - D_s z compacted IN PLACE into the packed low-resolution plane,
// v = IFFT2'((s2 + r2) / (s2 + r2 Lambda) FFT2' rho), D_s^T v expanded in place, g = IFFT2(conj(h^) FFT2(D_s^T v)).
// The low-resolution geometry keeps the full plane's n, so the one twiddle table serves both.
DC_HD dc_geom dc_sr_low(const dc_geom& g, int s, int lgs) {
    dc_geom l;
    l.h = g.h / s; l.m = g.m / s; l.lgh = g.lgh - lgs; l.lgm = g.lgm - lgs; l.p = l.m + 1; l.n = g.n;
    return l;
}

// v^ = (s2 + r2) / (s2 + r2 Lambda) rho^ on the low-resolution half spectrum [H/s][W/(2s) + 1]; denominator 0: 0
struct dc_sr_solve_filter {
    const double* lam;
    double s2, r2;
    DC_HD dc2 operator()(int idx, dc2 x) const {
        const double den = s2 + r2 * lam[idx];
        if (den == 0.0) return dc_make(0.0, 0.0);
        return dc_scale(x, (s2 + r2) / den);
    }
};

// An item is two neighbouring elements of the packed low-resolution plane: 4 real samples (i, 4 jj .. 4 jj + 3), which lie
// at the full plane's (s i, s (4 jj + e)): row s i, packed column (s / 2) (4 jj + e), real part.  Item `it` lives at low
// elements i p' + 2 jj (+ 1) and reads full elements >= s i p + 2 s jj >= i p' + 2 jj: no item reads below its own place,
// and the places rise with `it`.  So rounds of nthr items in rising order - read, barrier, write - never overwrite what a
// later round reads; the expansion runs the rounds in falling order by the same argument.

// rho = y - inv * (unscaled z)[s i][s j], compacted: on return z holds the packed low-resolution plane of geometry gl.
// y(i, col, v): the 4 measurement samples (i, col .. col + 3) of this plane.
template <class Y>
DC_HD void dc_sr_residual(dc2* z, const dc_geom& g, const dc_geom& gl, int s, double inv, const Y& y, int tid, int nthr) {
    const int per = gl.m >> 1, lgper = gl.lgm - 1, items = gl.h * per, hs = s >> 1;
    for (int base = 0; base < items; base += nthr) {
        const int it = base + tid;
        const bool on = it < items;
        double rho[4] = {0.0, 0.0, 0.0, 0.0};
        int at = 0;
        if (on) {
            const int i = it >> lgper, jj = it & (per - 1);
            y(i, 4 * jj, rho);
            const dc2* row = z + (s * i) * g.p + hs * 4 * jj;
            for (int e = 0; e < 4; ++e) rho[e] -= row[hs * e].x * inv;
            at = i * gl.p + 2 * jj;
        }
        DC_SYNC();
        if (on) {
            z[at] = dc_make(rho[0], rho[1]);
            z[at + 1] = dc_make(rho[2], rho[3]);
        }
    }
    DC_SYNC();
}

// the reverse: z holds the (unscaled) packed low-resolution plane v; on return the packed full plane D_s^T (inv * v)
DC_HD void dc_sr_zero_insert(dc2* z, const dc_geom& g, const dc_geom& gl, int s, double inv, int tid, int nthr) {
    const int per = gl.m >> 1, lgper = gl.lgm - 1, items = gl.h * per, hs = s >> 1;
    for (int base = ((items - 1) / nthr) * nthr; base >= 0; base -= nthr) {
        const int it = base + tid;
        const bool on = it < items;
        const int i = it >> lgper, jj = it & (per - 1);
        dc2 a = dc_make(0.0, 0.0), b = a;
        if (on) {
            a = z[i * gl.p + 2 * jj];
            b = z[i * gl.p + 2 * jj + 1];
        }
        DC_SYNC();
        if (on) {
            // the item's block of the full plane: s rows x 2 s packed columns; the blocks tile the plane
            const double v[4] = {a.x * inv, a.y * inv, b.x * inv, b.y * inv};
            dc2* blk = z + (s * i) * g.p + 2 * s * jj;
            for (int r = 0; r < s; ++r)
                for (int c = 0; c < 2 * s; ++c)
                    blk[r * g.p + c] = dc_make(r == 0 && (c & (hs - 1)) == 0 ? v[c / hs] : 0.0, 0.0);
        }
    }
    DC_SYNC();
}

// A x: the (unscaled) blurred plane in z, decimated; out(i, col, v) takes the 4 low-resolution samples (i, col .. col + 3)
template <class O>
DC_HD void dc_sr_decimate(const dc2* z, const dc_geom& g, const dc_geom& gl, int s, double inv, const O& out, int tid, int nthr) {
    const int per = gl.m >> 1, lgper = gl.lgm - 1, hs = s >> 1;
    DC_FOR(it, gl.h * per) {
        const int i = it >> lgper, jj = it & (per - 1);
        const dc2* row = z + (s * i) * g.p + hs * 4 * jj;
        double v[4];
        for (int e = 0; e < 4; ++e) v[e] = row[hs * e].x * inv;
        out(i, 4 * jj, v);
    }
    DC_SYNC();
}

// D_s^T r straight from memory: in(i, col, v) hands the 4 low-resolution samples (i, col .. col + 3)
template <class I>
DC_HD void dc_sr_spread(dc2* z, const dc_geom& g, const dc_geom& gl, int s, const I& in, int tid, int nthr) {
    const int per = gl.m >> 1, lgper = gl.lgm - 1, hs = s >> 1;
    DC_FOR(it, gl.h * per) {
        const int i = it >> lgper, jj = it & (per - 1);
        double v[4];
        in(i, 4 * jj, v);
        dc2* blk = z + (s * i) * g.p + 2 * s * jj;
        for (int r = 0; r < s; ++r)
            for (int c = 0; c < 2 * s; ++c)
                blk[r * g.p + c] = dc_make(r == 0 && (c & (hs - 1)) == 0 ? v[c / hs] : 0.0, 0.0);
    }
    DC_SYNC();
}
