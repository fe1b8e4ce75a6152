// Host check of the super-resolution per-plane arithmetic of csrc/deconv_core.h ("Super-resolution"): the
// same text the kernels of csrc/deconv.hip run, compiled for the host with one "thread" and no barrier, against the three
// steps written with a direct O(N^2) DFT.  No GPU, no Python:
//   clang++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -Ipsld_amd/csrc \
//       tools/sr_host_check.cpp -o sr_host_check && ./sr_host_check
// Exit status 0 and "ok" when every shape is within 1e-11 of the plane's magnitude; the sanitizers watch the in-place
// compaction and expansion of the plane storage.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "deconv_core.h"

typedef std::complex<double> cd;
static const double PI = 3.14159265358979323846;

static double rnd() { return (double)std::rand() / RAND_MAX - 0.5; }

// direct 2-D DFT of an h x w array (sign -1 forward, +1 inverse with the 1 / hw)
static std::vector<cd> dft2(const std::vector<cd>& x, int h, int w, int sign) {
    std::vector<cd> t((size_t)h * w), o((size_t)h * w);
    for (int r = 0; r < h; ++r)
        for (int k = 0; k < w; ++k) {
            cd a = 0;
            for (int j = 0; j < w; ++j) a += x[(size_t)r * w + j] * std::polar(1.0, sign * 2 * PI * ((long long)j * k % w) / w);
            t[(size_t)r * w + k] = a;
        }
    for (int k1 = 0; k1 < h; ++k1)
        for (int k = 0; k < w; ++k) {
            cd a = 0;
            for (int r = 0; r < h; ++r) a += t[(size_t)r * w + k] * std::polar(1.0, sign * 2 * PI * ((long long)r * k1 % h) / h);
            o[(size_t)k1 * w + k] = sign > 0 ? a / (double)(h * w) : a;
        }
    return o;
}

static int lg2(int n) {
    int l = 0;
    while ((1 << l) < n) ++l;
    return l;
}

struct load_y {
    const double* y;
    int wl;
    void operator()(int i, int col, double (&v)[4]) const {
        for (int e = 0; e < 4; ++e) v[e] = y[(size_t)i * wl + col + e];
    }
};
struct store_y {
    double* y;
    int wl;
    void operator()(int i, int col, const double (&v)[4]) const {
        for (int e = 0; e < 4; ++e) y[(size_t)i * wl + col + e] = v[e];
    }
};

static void pack(std::vector<dc2>& z, const dc_geom& g, const std::vector<double>& x) {
    for (int r = 0; r < g.h; ++r)
        for (int j = 0; j < g.m; ++j) z[(size_t)r * g.p + j] = dc_make(x[(size_t)r * 2 * g.m + 2 * j], x[(size_t)r * 2 * g.m + 2 * j + 1]);
}

static double check(int h, int w, int s, double s2, double r2, bool zero_lam) {
    const int hl = h / s, wl = w / s, tid = 0, nthr = 1;
    const dc_geom g = dc_geometry(h, w, lg2(h), lg2(w)), gl = dc_sr_low(g, s, lg2(s));
    // a random 5 x 5 kernel on the torus, its spectrum by the direct DFT, Lambda by the alias sum
    std::vector<cd> k((size_t)h * w, 0.0), x((size_t)h * w), y((size_t)hl * wl);
    for (int i = -2; i <= 2; ++i)
        for (int j = -2; j <= 2; ++j) k[(size_t)((i + h) % h) * w + (j + w) % w] += rnd();
    for (auto& v : x) v = rnd();
    for (auto& v : y) v = rnd();
    const std::vector<cd> hh = dft2(k, h, w, -1);
    std::vector<double> lam_full((size_t)hl * wl, 0.0);
    for (int m1 = 0; m1 < hl; ++m1)
        for (int m2 = 0; m2 < wl; ++m2) {
            double a = 0;
            for (int p = 0; p < s; ++p)
                for (int q = 0; q < s; ++q) a += std::norm(hh[(size_t)(m1 + p * hl) * w + m2 + q * wl]);
            lam_full[(size_t)m1 * wl + m2] = zero_lam && (m1 + m2) % 3 == 1 ? 0.0 : a / (s * s);
        }
    if (zero_lam)  // keep Lambda symmetric: Lambda[-m] = Lambda[m]
        for (int m1 = 0; m1 < hl; ++m1)
            for (int m2 = 0; m2 < wl; ++m2)
                lam_full[(size_t)((hl - m1) % hl) * wl + (wl - m2) % wl] = lam_full[(size_t)m1 * wl + m2];
    // the reference: three steps with the direct DFT
    std::vector<cd> xf = dft2(x, h, w, -1);
    for (size_t i = 0; i < xf.size(); ++i) xf[i] *= hh[i];
    const std::vector<cd> zr = dft2(xf, h, w, +1);
    std::vector<cd> rho((size_t)hl * wl);
    for (int i = 0; i < hl; ++i)
        for (int j = 0; j < wl; ++j) rho[(size_t)i * wl + j] = y[(size_t)i * wl + j] - zr[(size_t)(s * i) * w + s * j].real();
    std::vector<cd> rf = dft2(rho, hl, wl, -1);
    for (size_t i = 0; i < rf.size(); ++i) {
        const double den = s2 + r2 * lam_full[i];
        rf[i] = den == 0.0 ? cd(0.0) : rf[i] * ((s2 + r2) / den);
    }
    const std::vector<cd> v = dft2(rf, hl, wl, +1);
    std::vector<cd> up((size_t)h * w, 0.0);
    for (int i = 0; i < hl; ++i)
        for (int j = 0; j < wl; ++j) up[(size_t)(s * i) * w + s * j] = v[(size_t)i * wl + j].real();
    std::vector<cd> uf = dft2(up, h, w, -1);
    for (size_t i = 0; i < uf.size(); ++i) uf[i] *= std::conj(hh[i]);
    const std::vector<cd> want = dft2(uf, h, w, +1);
    // the code under test: exactly sized storage, so that the sanitizer sees any step outside it
    std::vector<dc2> z((size_t)dc_plane_elems(g)), tw((size_t)g.n / 2), hhalf((size_t)h * (g.m + 1));
    std::vector<double> lam((size_t)hl * (gl.m + 1)), xr((size_t)h * w), yr((size_t)hl * wl);
    for (int r = 0; r < h; ++r)
        for (int c = 0; c <= g.m; ++c) hhalf[(size_t)r * (g.m + 1) + c] = dc_make(hh[(size_t)r * w + c].real(), hh[(size_t)r * w + c].imag());
    for (int r = 0; r < hl; ++r)
        for (int c = 0; c <= gl.m; ++c) lam[(size_t)r * (gl.m + 1) + c] = lam_full[(size_t)r * wl + c];
    for (size_t i = 0; i < x.size(); ++i) xr[i] = x[i].real();
    for (size_t i = 0; i < y.size(); ++i) yr[i] = y[i].real();
    const double inv = 1.0 / (h * g.m), invl = 1.0 / (hl * gl.m);
    dc_twiddles(tw.data(), g, tid, nthr);
    pack(z, g, xr);
    dc_forward(z.data(), tw.data(), g, tid, nthr);
    dc_filter<false>(z.data(), tw.data(), g, dc_apply_filter{hhalf.data(), false}, nullptr, tid, nthr);
    dc_inverse(z.data(), tw.data(), g, tid, nthr);
    // A x on the way: the decimation of the apply kernel
    std::vector<double> ax((size_t)hl * wl);
    dc_sr_decimate(z.data(), g, gl, s, inv, store_y{ax.data(), wl}, tid, nthr);
    double err = 0, mag = 0;
    for (int i = 0; i < hl; ++i)
        for (int j = 0; j < wl; ++j) {
            err = std::fmax(err, std::fabs(ax[(size_t)i * wl + j] - zr[(size_t)(s * i) * w + s * j].real()));
            mag = std::fmax(mag, std::fabs(ax[(size_t)i * wl + j]));
        }
    dc_sr_residual(z.data(), g, gl, s, inv, load_y{yr.data(), wl}, tid, nthr);
    dc_forward(z.data(), tw.data(), gl, tid, nthr);
    dc_filter<false>(z.data(), tw.data(), gl, dc_sr_solve_filter{lam.data(), s2, r2}, nullptr, tid, nthr);
    dc_inverse(z.data(), tw.data(), gl, tid, nthr);
    dc_sr_zero_insert(z.data(), g, gl, s, invl, tid, nthr);
    dc_forward(z.data(), tw.data(), g, tid, nthr);
    dc_filter<false>(z.data(), tw.data(), g, dc_apply_filter{hhalf.data(), true}, nullptr, tid, nthr);
    dc_inverse(z.data(), tw.data(), g, tid, nthr);
    for (int r = 0; r < h; ++r)
        for (int j = 0; j < g.m; ++j) {
            const dc2 a = z[(size_t)r * g.p + j];
            err = std::fmax(err, std::fabs(a.x * inv - want[(size_t)r * w + 2 * j].real()));
            err = std::fmax(err, std::fabs(a.y * inv - want[(size_t)r * w + 2 * j + 1].real()));
            mag = std::fmax(mag, std::fabs(want[(size_t)r * w + 2 * j].real()));
        }
    // A^T r straight from memory: the spread of the apply kernel against the zero insertion
    std::vector<dc2> z2((size_t)dc_plane_elems(g));
    dc_sr_spread(z2.data(), g, gl, s, load_y{yr.data(), wl}, tid, nthr);
    for (int r = 0; r < h; ++r)
        for (int c = 0; c < w; ++c) {
            const dc2 a = z2[(size_t)r * g.p + c / 2];
            const double got = c % 2 ? a.y : a.x, exp = r % s == 0 && c % s == 0 ? yr[(size_t)(r / s) * wl + c / s] : 0.0;
            if (got != exp) err = 1.0;
        }
    std::printf("%3d x %3d s = %d s2 = %g%s: max error %.2e (max |value| %.2e)\n", h, w, s, s2, zero_lam ? " Lambda with zeros" : "", err, mag);
    return err / (mag > 1.0 ? mag : 1.0);
}

int main() {
    std::srand(7);
    const int shapes[][3] = {{8, 8, 2}, {16, 16, 4}, {8, 16, 2}, {16, 8, 2}, {32, 16, 4}, {16, 64, 4}, {32, 32, 2}, {32, 32, 4}, {64, 32, 2}};
    double worst = 0;
    for (const auto& sh : shapes) {
        worst = std::fmax(worst, check(sh[0], sh[1], sh[2], 0.0025, 0.3, false));
        worst = std::fmax(worst, check(sh[0], sh[1], sh[2], 0.0, 0.3, true));
    }
    std::printf("%s: worst relative error %.2e\n", worst <= 1e-11 ? "ok" : "FAILED", worst);
    return worst <= 1e-11 ? 0 : 1;
}
