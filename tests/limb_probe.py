"""Exact probes of the three-limb arithmetic (math mode 'bf16x6') and its CPU model: what the limb kernels compute, bit for bit.

The contract (csrc/conv_split.hip): an fp32 operand is split exactly into hi + mid + lo (bf16 each) and a product is
accumulated in fp32 from the six limb products lo*hi, hi*lo, mid*mid, mid*hi, hi*mid, hi*hi (A-side limb * B-side limb).
``six_limb_einsum`` is the three-limb twin of ``x3_ref.two_limb_einsum``: the six products in fp64, any of them left out
(``drop=``) or counted twice (``double=``) on request.  In this file the A side is the FIRST einsum operand - the activation
/ left matrix / output gradient of a launch - and the B side the second (weights / right matrix / layer input).

Probe values.  Three classes of (A-side, B-side) values light up all six products between them:
    class 0:  1 + 2^-9 + 2^-18  *  power of two        hi*hi, mid*hi, lo*hi
    class 1:  power of two      *  1 + 2^-9 + 2^-18    hi*hi, hi*mid, hi*lo
    class 2:  1 + 2^-9          *  1 + 2^-11           hi*hi, hi*mid, mid*hi, mid*mid
Every element carries its own sign and power of two (2^e, |e| <= 10 per side, so a product within 2^+-20).  The builder
checks with ``split3`` that the limbs are the intended ones and that no value sits on a round-to-even tie.  One launch holds
one class; the launches of a case take the classes in turn.

Operands are arranged so that one output element is ONE product (a scaled permutation against a dense matrix, single-tap
weights, inputs on a stride-3 pixel lattice, one pixel per channel), so every limb product and every fp32 partial sum is
exactly representable whatever the summation order, and the kernel's output must EQUAL the model.

Admissibility (``Launch.margins``; a case that fails is a bug of the probe, never a tolerance):
  * contraction (the MFMA accumulation): over the limb products that reach one output element, S = the sum of their absolute
    values and q = a power of two that divides them all (a lower bound: the reciprocal of the sum of the reciprocals of the
    products' own quanta - exact when one term dominates, never too large); S < 2^24 q.
  * the fp32 Winograd transforms (input, weight, output; the weight gradient's G^T dU G): the same with the transform's
    terms (coefficient * value).  For the transforms that SUM several non-zero values (the output transform, G^T dU G) q is
    the exact minimum of the terms' quanta and the bound is the tight one: a partial sum of any subset in any order is a
    multiple of q of magnitude at most max(P, N) (P / N: the sums of the positive / negative terms), so all of them are
    exact iff max(P, N) < 2^24 q.  The plain sum of absolute values P + N would turn down class 2 on the Winograd corner
    tiles (terms xw * {1, -1/2 x4, 1/4 x4}: P + N = 4 |xw|, q = q(xw) / 4, |xw| / q(xw) = 2^20 (1 + 2^-9) (1 + 2^-11))
    by a factor 1.003 although no subset of them sums past 2 |xw|.
  * the model's value is itself an fp32 number.
No GPU here, and nothing outside the repository."""
import functools
import math

import torch
import torch.nn.functional as F

from tests import x3_ref as X
from tests import x3_train_ref as XT

LIMBS = ("hi", "mid", "lo")
PRODUCTS = ("lo*hi", "hi*lo", "mid*mid", "mid*hi", "hi*mid", "hi*hi")        # the documented six, smallest first
X3_PRODUCTS = ("mid*hi", "hi*mid", "hi*hi")                                   # the two-limb launches (math mode 'bf16x3')
AIMED = ("lo*hi", "hi*lo", "mid*mid")           # the product only class 0 / 1 / 2 lights
TWO24 = float(2 ** 24)

_T, _N = 2.0 ** -9, 2.0 ** -18
CLASS_LIMBS = (((1.0, _T, _N), (1.0, 0.0, 0.0)),
               ((1.0, 0.0, 0.0), (1.0, _T, _N)),
               ((1.0, _T, 0.0), (1.0, 2.0 ** -11, 0.0)))
CLASS_LIT = (("hi*hi", "mid*hi", "lo*hi"), ("hi*hi", "hi*mid", "hi*lo"), ("hi*hi", "hi*mid", "mid*hi", "mid*mid"))
_AT = torch.tensor([[1.0, 1.0, 1.0, 0.0], [0.0, 1.0, -1.0, -1.0]], dtype=torch.float64)      # output transform A^T
_GT = XT._G.t().contiguous()                                                                   # G^T [3][4]


# ---- the arithmetic ------------------------------------------------------------------------------------------------------
def _mm(a, b):
    """a [m][k] @ b[n][k]^T in fp64; a mostly-zero operand goes through a sparse product (the same terms, fewer zeros)."""
    if a.numel() >= 4096 and b.numel() >= 4096:
        na, nb = int(torch.count_nonzero(a)), int(torch.count_nonzero(b))
        if na * 16 <= a.numel() and na <= nb:
            return torch.sparse.mm(a.to_sparse(), b.t().contiguous())
        if nb * 16 <= b.numel():
            return torch.sparse.mm(b.to_sparse(), a.t().contiguous()).t()
    return a @ b.t()


def _contract(eq, a, b):
    return _mm(a, b) if eq == "mk,nk->mn" else torch.einsum(eq, a, b)


def _live_k(eq, a, b):
    """The operands of a matrix product without the k at which one of them is all zero (no term there)."""
    if eq == "mk,nk->mn" and a.numel() >= 4096:
        keep = (a != 0).any(0) & (b != 0).any(0)
        if int(keep.sum()) * 2 <= keep.numel():
            keep = keep.nonzero().flatten()
            return a[:, keep].contiguous(), b[:, keep].contiguous()
    return a, b


def limb_products(eq, a, b, products=PRODUCTS):
    """{name: einsum(eq, A limb, B limb) in fp64} for the named limb products of fp32 operands ``a`` and ``b``."""
    a, b = _live_k(eq, a, b)
    al = dict(zip(LIMBS, (t.double() for t in X.split3(a))))
    bl = dict(zip(LIMBS, (t.double() for t in X.split3(b))))
    return {p: _contract(eq, al[p.split("*")[0]], bl[p.split("*")[1]]) for p in products}


def sum_products(prods, products=PRODUCTS, drop=None, double=None):
    """Sum of the named products in the fixed order of ``products`` (smallest first), without ``drop``, ``double`` twice."""
    out = None
    for p in products:
        if p == drop:
            continue
        t = prods[p] * 2.0 if p == double else prods[p]
        out = t.clone() if out is None else out + t
    return out


def six_limb_einsum(eq, a, b, drop=None, double=None, products=PRODUCTS):
    """einsum(eq, a, b) in three-limb arithmetic, fp64 result: split3 of both operands, the six documented limb products.
    ``drop`` names one product to leave out, ``double`` one to count twice (CPU tests and failure messages only)."""
    want = set(products) | ({double} if double else set())
    return sum_products(limb_products(eq, a, b, tuple(p for p in PRODUCTS if p in want)), products, drop, double)


def quantum(v):
    """Largest power of two that divides each fp64 value (inf for 0)."""
    v = v.double()
    m, e = torch.frexp(v)
    mi = (m.abs() * float(2 ** 53)).to(torch.int64)
    low = (mi & -mi).double()
    return torch.where(v == 0, torch.full_like(v, math.inf), torch.ldexp(low, e - 53))


def _inv_quantum(v):
    return 1.0 / quantum(v)         # 0 for a zero value


def contraction_margin(eq, a, b, products=PRODUCTS):
    """max over the lit output elements of S / (2^24 q) for the limb products of einsum(eq, a, b): admissible iff < 1."""
    a, b = _live_k(eq, a, b)
    al = dict(zip(LIMBS, (t.double() for t in X.split3(a))))
    bl = dict(zip(LIMBS, (t.double() for t in X.split3(b))))
    s = invq = 0.0
    for p in products:
        i, j = p.split("*")
        s = s + _contract(eq, al[i].abs(), bl[j].abs())
        invq = invq + _contract(eq, _inv_quantum(al[i]), _inv_quantum(bl[j]))
    return float((s * invq).max()) / TWO24


def sandwich_margins(lm, x):
    """y[a][b] = sum_rs lm[a][r] lm[b][s] x[r][s][...] formed in fp32 from exact values x: (tight, plain) margins - the
    max over the lit outputs of max(P, N) / (2^24 q) and of (P + N) / (2^24 q), q the exact minimum of the terms' quanta."""
    qx = quantum(x)
    xp, xn = x.clamp(min=0.0), (-x).clamp(min=0.0)
    tight = plain = 0.0
    for a in range(lm.shape[0]):
        for b in range(lm.shape[0]):
            pos = torch.zeros_like(x[0, 0])
            neg = torch.zeros_like(pos)
            q = torch.full_like(pos, math.inf)
            for r in range(lm.shape[1]):
                for s in range(lm.shape[1]):
                    c = float(lm[a, r] * lm[b, s])
                    if c == 0.0:
                        continue
                    pos += abs(c) * (xp[r, s] if c > 0 else xn[r, s])
                    neg += abs(c) * (xn[r, s] if c > 0 else xp[r, s])
                    q = torch.minimum(q, qx[r, s] * abs(c))
            lit = torch.isfinite(q)
            if bool(lit.any()):
                tight = max(tight, float((torch.maximum(pos, neg)[lit] / q[lit]).max()) / TWO24)
                plain = max(plain, float(((pos + neg)[lit] / q[lit]).max()) / TWO24)
    return tight, plain


def _exact_in_f32(t):
    return bool(torch.equal(t.float().double(), t))


# ---- probe values --------------------------------------------------------------------------------------------------------
def _on_tie(x):
    """True where rne_bf16(x) had to break a tie (the remainder is exactly half a bf16 ulp of x)."""
    x = x.double()
    r = x - x.float().to(torch.bfloat16).double()
    _, e = torch.frexp(x)
    return (r != 0) & (r.abs() == torch.ldexp(torch.ones_like(x), e - 9))


def probe_values(shape, cls, side, seed):
    """fp32 tensor of ``shape``: the class's A-side (side 0) or B-side (side 1) value times +-2^e, e in [-10, 10], sign and
    exponent drawn per element.  Asserts the three limbs are the intended ones and that no split meets a tie."""
    g = torch.Generator().manual_seed(seed * 7 + cls * 2 + side + 1)
    e = torch.randint(-10, 11, shape, generator=g)
    sg = torch.randint(0, 2, shape, generator=g).double() * 2.0 - 1.0
    scale = torch.ldexp(sg, e)
    limbs = CLASS_LIMBS[cls][side]
    v64 = scale * sum(limbs)
    v = v64.float()
    assert torch.equal(v.double(), v64)
    got = X.split3(v)
    for want, have in zip(limbs, got):
        assert torch.equal(have.double(), scale * want), (cls, side, want)
    r = v64 - got[0].double()
    assert not bool(_on_tie(v64).any()) and not bool(_on_tie(r).any()) and not bool(_on_tie(r - got[1].double()).any())
    return v


# ---- launches and cases --------------------------------------------------------------------------------------------------
class Launch:
    """One launch of a case: ``inp`` = the kernel's operands (CPU fp32, in the layouts the family's adapter wants), ``cls`` the
    probe class.  ``kind``: 'mm' (a [m][k], b [n][k] -> [m][n]; batched: lists), 'wino' (x NCHW, w = effective OIHW -> NHWC
    rows [b*h*w][cout]) or 'wwino' (dy, x NCHW -> [cout][cin*9]).  The model's output is always the 2-D (batched: 3-D) tensor
    in the kernel's own output order."""

    def __init__(self, kind, cls, inp, a=None, b=None):
        self.kind, self.cls, self.inp, self._a, self._b = kind, cls, inp, a, b       # a / b: tensors, lists or thunks
        self._prods = self._margins = None

    @property
    def a(self):
        return self._a() if callable(self._a) else self._a

    @property
    def b(self):
        return self._b() if callable(self._b) else self._b

    # -- the six (named) products of the output, fp64 --
    def prods(self):
        if self._prods is not None:
            return self._prods
        out = getattr(self, "_prods_" + self.kind)()
        if out["hi*hi"].numel() <= 1 << 20:          # the large outputs are formed again on demand rather than kept
            self._prods = out
        return out

    def expected(self, products=PRODUCTS, drop=None, double=None, prods=None):
        return sum_products(prods if prods is not None else self.prods(), products, drop, double)

    def _prods_mm(self):
        if isinstance(self._a, list):
            per = [limb_products("mk,nk->mn", a, b) for a, b in zip(self.a, self.b)]
            return {p: torch.stack([d[p] for d in per], 0) for p in PRODUCTS}
        return limb_products("mk,nk->mn", self.a, self.b)

    def _wino_operands(self):
        """(V gathered [16][tiles][cout], U gathered [16][cout], V, U, V's shape): an output channel has one non-zero input
        channel, so sum_c V[p][t][c] U[p][o][c] is the one term V[p][t][c(o)] U[p][o][c(o)]."""
        x, w = self.inp["x"], self.inp["w"]
        v5 = X.wino_v(x)                                         # fp32 [16][B][H/2][W/2][C]
        v, u = v5.reshape(16, -1, x.shape[1]), X.wino_u(w)
        live = (u != 0).any(0)                                   # [cout][cin]
        assert int(live.sum(1).max()) <= 1
        c = live.float().argmax(1)
        return v[:, :, c], u[:, torch.arange(u.shape[1]), c], v, u, v5.shape

    def _prods_wino(self):
        vg, ug, _, _, vs = self._wino_operands()
        out = {}
        for p, m in limb_products("pto,po->pto", vg, ug).items():
            out[p] = _wino_output(m, vs[1], vs[2], vs[3])
        return out

    def _wwino_operands(self):
        dy, x = self.inp["dy"], self.inp["x"]
        img = ((dy != 0).flatten(1).any(1) & (x != 0).flatten(1).any(1)).nonzero().flatten()      # the images with a term
        dy, x = dy[img], x[img]
        m, v = XT.wino_m(dy).reshape(16, -1, dy.shape[1]), XT.wino_v_cols_first(x).reshape(16, -1, x.shape[1])
        keep = ((m != 0).any(2).any(0) & (v != 0).any(2).any(0)).nonzero().flatten()          # tiles with a term
        return m[:, keep].contiguous(), v[:, keep].contiguous()

    def _prods_wwino(self):
        m, v = self._wwino_operands()
        out = {}
        for p, du in limb_products("pto,ptc->poc", m, v).items():
            du = du.reshape(4, 4, du.shape[1], du.shape[2])
            out[p] = torch.einsum("ia,jb,ijoc->ocab", XT._G, XT._G, du).reshape(du.shape[2], -1)
        return out

    # -- admissibility: {stage: margin}, every one < 1 --
    def margins(self, products=PRODUCTS):
        if self._margins is None:
            self._margins = getattr(self, "_margins_" + self.kind)(products)
            assert _exact_in_f32(self.expected(products)), "the model's value is no fp32 number"
        return self._margins

    def _margins_mm(self, products):
        ab = zip(self.a, self.b) if isinstance(self._a, list) else [(self.a, self.b)]
        return {"contraction": max(contraction_margin("mk,nk->mn", a, b, products) for a, b in ab)}

    def _margins_wino(self, products):
        x, w = self.inp["x"], self.inp["w"]
        vg, ug, v, u, vs = self._wino_operands()
        bt = torch.tensor([[1.0, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
        d = F.pad(x.double(), (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2).permute(4, 5, 0, 2, 3, 1)
        o = torch.arange(w.shape[0])
        c = (u != 0).any(0).float().argmax(1)                    # the one live input channel of every output channel
        g = torch.zeros(4, 4, w.shape[0], dtype=torch.float64)
        g[:3, :3] = w.double()[o, c].permute(1, 2, 0)
        gm = torch.cat([XT._G, torch.zeros(4, 1, dtype=torch.float64)], 1)
        out = {"input transform": sandwich_margins(bt, d)[1], "weight transform": sandwich_margins(gm, g)[1],
               "contraction": contraction_margin("pto,po->pto", vg, ug, products)}
        # the transforms in fp32 (the kernels' operation order) are the exact ones
        assert torch.equal(v.double().reshape(4, 4, *d.shape[2:]), torch.einsum("ir,js,rs...->ij...", bt, bt, d))
        assert torch.equal(ug.double().reshape(4, 4, -1), torch.einsum("ir,js,rs...->ij...", gm, gm, g))
        m = sum_products(limb_products("pto,po->pto", vg, ug), products)
        assert _exact_in_f32(m)
        out["output transform (tight)"], out["output transform (plain sum, informative)"] = \
            sandwich_margins(_AT, m.reshape(4, 4, m.shape[1], m.shape[2]))
        return out

    def _margins_wwino(self, products):
        dy, x = self.inp["dy"], self.inp["x"]
        m, v = self._wwino_operands()
        # single non-zero pixel per 2x2 / 4x4 tile and channel: the transforms copy it with a sign
        t = dy.reshape(dy.shape[0], dy.shape[1], dy.shape[2] // 2, 2, dy.shape[3] // 2, 2)
        assert int((t != 0).sum(dim=(3, 5)).max()) <= 1, "two output-gradient pixels in one 2x2 tile"
        xt = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)
        assert int((xt != 0).sum(dim=(4, 5)).max()) <= 1, "two input pixels in one 4x4 tile"
        out = {"contraction": contraction_margin("pto,ptc->poc", m, v, products)}
        du = sum_products(limb_products("pto,ptc->poc", m, v), products)
        assert _exact_in_f32(du)
        out["G^T dU G (tight)"], out["G^T dU G (plain sum, informative)"] = \
            sandwich_margins(_GT, du.reshape(4, 4, du.shape[1], du.shape[2]))
        return out

    def admissible(self):
        return all(v < 1.0 for k, v in self.margins().items() if "informative" not in k)

    # -- K positions with a term (a and b both non-zero somewhere) --
    def k_used(self):
        if self.kind == "mm":
            ab = zip(self.a, self.b) if isinstance(self._a, list) else [(self.a, self.b)]
            u = None
            for a, b in ab:
                t = (a != 0).any(0) & (b != 0).any(0)
                u = t if u is None else u | t
            return u
        if self.kind == "wino":
            x, w = self.inp["x"], self.inp["w"]
            cols = F.unfold((x != 0).float(), 3, padding=1)                    # [B][ci*9][L]
            return (cols != 0).any(2).any(0) & (w.reshape(w.shape[0], -1) != 0).any(0)
        dy, x = self.inp["dy"], self.inp["x"]                  # K = the 2x2 tiles
        cols = F.unfold((x != 0).float(), 3, padding=1)
        pix = ((dy != 0).any(1).reshape(-1)) & (cols != 0).any(1).reshape(-1)
        b, _, h, w = dy.shape
        return pix.reshape(b, h // 2, 2, w // 2, 2).any(4).any(2).reshape(-1)


def _wino_output(m, b, th, tw):
    """Y = A^T M A of [16][tiles][cout] -> NHWC rows [b*h*w][cout], fp64."""
    co = m.shape[-1]
    y = torch.einsum("ir,js,rsto->tijo", _AT, _AT, m.reshape(4, 4, -1, co))           # [tiles][2][2][co]
    return y.reshape(b, th, tw, 2, 2, co).permute(0, 1, 3, 2, 4, 5).reshape(b * th * 2 * tw * 2, co)


class Case:
    def __init__(self, family, name, params, launches):
        self.family, self.name, self.params, self.launches = family, name, params, launches

    def __repr__(self):
        return f"{self.family}:{self.name}"


def _pix(k, h, w):
    return k // (h * w), (k // w) % h, k % w


def _interior(b, h, w):
    return [(i * h + y) * w + x for i in range(b) for y in range(1, h - 1) for x in range(1, w - 1)]


# -- GEMMs: one operand dense in probe values, the other a scaled permutation --
def _perm_operand(rows, k, shift, cls, side, seed):
    """[rows][k] with one non-zero per row, at column (row + shift) % k."""
    t = torch.zeros(rows, k)
    r = torch.arange(rows)
    t[r, (r + shift) % k] = probe_values((rows,), cls, side, seed)
    return t


def gemm_launches(m, n, k, way, batch=None, seed=0):
    """way 'dense_a': a dense, b[n][k] a scaled permutation; 'dense_b': the other way round.  Rounds shift the permutation
    until every k has been used; each round runs the three classes."""
    rows = n if way == "dense_a" else m
    out = []
    for rnd in range(-(-k // rows)):
        for cls in range(3):
            def one(i):
                s = seed + 31 * len(out) + 1009 * i
                if way == "dense_a":
                    return probe_values((m, k), cls, 0, s), _perm_operand(n, k, rnd * rows + i, cls, 1, s)
                return _perm_operand(m, k, rnd * rows + i, cls, 0, s), probe_values((n, k), cls, 1, s)
            if batch is None:
                a, b = one(0)
            else:
                a, b = (list(t) for t in zip(*[one(i) for i in range(batch)]))
            out.append(Launch("mm", cls, {}, a, b))
    return out


# -- 3x3 convolutions (forward; the data gradient is the same kernel on other fragments) --
def _cols(x):
    """im2col of NCHW x: [b*h*w][ci*9] (row = NHWC pixel, column = ci*9 + tap)."""
    b, c = x.shape[:2]
    return F.unfold(x, 3, padding=1).permute(0, 2, 1).reshape(-1, c * 9)


def _single_tap_weights(co, cin, pos, cls, seed):
    """OIHW weights with one non-zero (c_in, tap) per output channel: flat position pos[o] = tap * cin + c_in."""
    w = torch.zeros(co, cin, 9)
    o = torch.arange(co)
    w[o, pos % cin, pos // cin] = probe_values((co,), cls, 1, seed)
    return w.reshape(co, cin, 3, 3)


def _lattice_mask(b, h, w, oy, ox):
    m = torch.zeros(b, 1, h, w, dtype=torch.bool)
    m[:, :, oy::3, ox::3] = True
    return m


def conv_launches(b, cin, co, h, w, way, seed=0):
    """'dense_x': input dense, one (c_in, tap) per output channel - position rounds walk all 9*cin weight positions, three
    more launches put every channel on the centre tap (the only tap that reaches every pixel) in each class.
    'dense_w': weights dense, the input has one non-zero channel per pixel of a stride-3 lattice; nine lattice offsets x
    three classes per round, the channels handed out in turn, rounds until every (tap, c_in) has met a pixel."""
    out = []
    o = torch.arange(co)
    if way == "dense_x":
        plan = [((o + r * co) % (9 * cin), r % 3) for r in range(-(-9 * cin // co))]
        plan += [(4 * cin + o % cin, c) for c in range(3)]
        for pos, cls in plan:
            s = seed + 17 * len(out)
            x, wt = probe_values((b, cin, h, w), cls, 0, s), _single_tap_weights(co, cin, pos, cls, s)
            out.append(Launch("mm", cls, {"x": x, "w": wt}, functools.partial(_cols, x), wt.reshape(co, -1)))
        return out
    wts = [probe_values((co, cin, 3, 3), cls, 1, seed + cls) for cls in range(3)]
    used = torch.zeros(cin * 9, dtype=torch.bool)
    counter = [0, 0]
    while not bool(used.all()):
        assert len(out) < 27 * 40, "the lattice never reaches every weight position"
        for cls in range(3):
            for off in range(9):
                mask = _lattice_mask(b, h, w, off // 3, off % 3)
                idx = mask.expand(b, 1, h, w).reshape(b, h, w).nonzero()
                # interior pixels meet all nine taps: they take the channels in turn; border pixels follow their own count
                inner = (idx[:, 1] > 0) & (idx[:, 1] < h - 1) & (idx[:, 2] > 0) & (idx[:, 2] < w - 1)
                rank = torch.where(inner, torch.cumsum(inner, 0) - 1 + counter[0], torch.cumsum(~inner, 0) - 1 + counter[1])
                ch = rank % cin
                counter = [counter[0] + int(inner.sum()), counter[1] + int((~inner).sum())]
                x = torch.zeros(b, cin, h, w)
                x[idx[:, 0], ch, idx[:, 1], idx[:, 2]] = probe_values((len(idx),), cls, 0, seed + 13 * len(out))
                la = Launch("mm", cls, {"x": x, "w": wts[cls], "wkey": cls}, functools.partial(_cols, x), wts[cls].reshape(co, -1))
                used |= la.k_used()
                out.append(la)
    return out


def wino_launches(b, cin, co, h, w, seed=0):
    """Both operands sparse: the input dense in channels on a stride-3 pixel lattice, one (c_in, tap) per output channel.
    27 launches (nine lattice offsets x three classes) with every channel on the centre tap reach every output element;
    position rounds (lattice offset (1, 1), where every tap lands inside) walk the 9*cin weight positions."""
    out = []
    o = torch.arange(co)
    plan = [(4 * cin + o % cin, cls, off) for cls in range(3) for off in range(9)]
    plan += [((o + r * co) % (9 * cin), r % 3, 4) for r in range(-(-9 * cin // co))]
    for pos, cls, off in plan:
        s = seed + 19 * len(out)
        x = probe_values((b, cin, h, w), cls, 0, s) * _lattice_mask(b, h, w, off // 3, off % 3)
        out.append(Launch("wino", cls, {"x": x, "w": _single_tap_weights(co, cin, pos, cls, s)}))
    return out


# -- weight gradients --
def wgrad_launches(b, cin, co, h, w, way, seed=0):
    """dw[co][ci][tap] = sum over pixels of dy[p][co] x[p + tap][ci].  'sparse_dy': one non-zero pixel per output channel, x
    dense; 'sparse_x': one non-zero pixel per input channel, dy dense.  Per class: rounds move the pixels over the whole K
    range, one more round puts them on interior pixels (all nine taps land inside)."""
    k = b * h * w
    ch = co if way == "sparse_dy" else cin
    c = torch.arange(ch)
    inner = torch.tensor(_interior(b, h, w))
    plans = [(c + r * ch) % k for r in range(-(-k // ch))] + [inner[(c * 5) % len(inner)]]
    out = []
    for pix in plans:
        for cls in range(3):
            s = seed + 23 * len(out)
            pb, py, px = _pix(pix, h, w)
            if way == "sparse_dy":
                dy = torch.zeros(b, co, h, w)
                dy[pb, c, py, px] = probe_values((co,), cls, 0, s)
                x = probe_values((b, cin, h, w), cls, 1, s)
            else:
                x = torch.zeros(b, cin, h, w)
                x[pb, c, py, px] = probe_values((cin,), cls, 1, s)
                dy = probe_values((b, co, h, w), cls, 0, s)
            out.append(Launch("mm", cls, {"dy": dy, "x": x}, dy.permute(1, 0, 2, 3).reshape(co, -1),
                              functools.partial(lambda t: _cols(t).t().contiguous(), x)))
    return out


_OFF9 = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def wwino_launches(b, cin, co, h, w, way, seed=0):
    """Winograd-domain weight gradient, both operands sparse.  'dy_pixel': in image i the output gradient is non-zero at one
    pixel p_i, in the channels co = i (mod b) only, and the input at one pixel per channel, p_i + offset[(ci + rotation) % 9]:
    dw[co][ci][tap] is the one product of image co % b, and nine rotations x three classes light every (co, ci, tap).
    'x_pixel': the roles swapped.  p_i walks the 2x2 tiles of its image (interior pixels only), so every K tile is used."""
    tiles = [(ty, tx) for ty in range(h // 2) for tx in range(w // 2)]
    out = []
    for l in range(27 * -(-len(tiles) // 27)):
        cls, rot = l % 3, (l // 3) % 9
        s = seed + 29 * l
        dy, x = torch.zeros(b, co, h, w), torch.zeros(b, cin, h, w)
        many, single = (x, dy) if way == "dy_pixel" else (dy, x)
        vs = probe_values((single.shape[1],), cls, 0 if single is dy else 1, s)
        vm = probe_values((b, many.shape[1]), cls, 0 if many is dy else 1, s + 1)
        cs, cm = torch.arange(single.shape[1]), torch.arange(many.shape[1])
        off = torch.tensor(_OFF9)[(cm + rot) % 9]
        for i in range(b):
            ty, tx = tiles[(l + 5 * i) % len(tiles)]
            sub = (l // len(tiles) + i) % 4
            py = min(max(2 * ty + sub // 2, 1), h - 2)
            px = min(max(2 * tx + sub % 2, 1), w - 2)
            mine = cs[cs % b == i]
            single[i, mine, py, px] = vs[mine]
            many[i, cm, py + off[:, 0], px + off[:, 1]] = vm[i]
        out.append(Launch("wwino", cls, {"dy": dy, "x": x}))
    return out


# ---- the case table (shared by the CPU and the GPU tests) ----------------------------------------------------------------
CONV_SHAPES = [(2, 64, 0, 128, 8, 8), (2, 64, 32, 128, 16, 16), (2, 32, 0, 128, 4, 8), (1, 256, 256, 256, 8, 8)]
WINO_SPLIT_SHAPE = (1, 256, 0, 256, 16, 16)
GEMM_SHAPES = [(256, 128, 64, 0), (640, 128, 96, 32), (16384, 256, 128, 0)]       # m, n, k1, k2; the last: eight waves
GEMM_TAIL_SHAPE = (130, 160, 160)                                                  # m, k, n
TN_SHAPES = [(128, 128, 192)]                                                      # m, n, k: six K tiles
TN_TAIL_SHAPES = [(160, 160, 192)]
BGEMM_SHAPE, BGEMM_TAIL_SHAPE, BGEMM_BATCH = (256, 128, 96), (256, 160, 96), 3
BGEMM_LAYOUTS = [(0, 1), (0, 0), (1, 0)]
WGRAD_SHAPES = [(2, 128, 64, 8, 8), (3, 128, 256, 16, 16)]                         # b, ci, co, h, w
WWINO_SHAPES = [(8, 128, 0, 256, 8, 8), (4, 128, 256, 256, 8, 8)]                  # b, c1, c2, co, h, w


def _shape_id(t):
    return "x".join(str(v) for v in t)


CASES = {}


def _register(family, name, params, builder):
    CASES[f"{family}:{name}"] = (family, name, params, builder)


for _s in CONV_SHAPES:
    for _way in ("dense_x", "dense_w"):
        _register("conv", f"{_shape_id(_s)}-{_way}", dict(shape=_s, way=_way),
                  functools.partial(conv_launches, _s[0], _s[1] + _s[2], _s[3], _s[4], _s[5], _way))
for _s in CONV_SHAPES + [WINO_SPLIT_SHAPE]:
    _register("wino", _shape_id(_s), dict(shape=_s, split=_s == WINO_SPLIT_SHAPE),
              functools.partial(wino_launches, _s[0], _s[1] + _s[2], _s[3], _s[4], _s[5]))
for _m, _n, _k1, _k2 in GEMM_SHAPES:
    for _way in ("dense_a", "dense_b"):
        _register("gemm", f"{_m}x{_n}x{_k1}+{_k2}-{_way}", dict(m=_m, n=_n, k1=_k1, k2=_k2, way=_way),
                  functools.partial(gemm_launches, _m, _n, _k1 + _k2, _way))
for _way in ("dense_a", "dense_b"):
    _m, _k, _n = GEMM_TAIL_SHAPE
    _register("gemm_tail", f"{_m}x{_k}x{_n}-{_way}", dict(m=_m, n=_n, k=_k, way=_way),
              functools.partial(gemm_launches, _m, _n, _k, _way))
    for _fam, _shapes in (("tn", TN_SHAPES), ("tn_tail", TN_TAIL_SHAPES)):
        for _m, _n, _k in _shapes:
            _register(_fam, f"{_m}x{_n}x{_k}-{_way}", dict(m=_m, n=_n, k=_k, way=_way),
                      functools.partial(gemm_launches, _m, _n, _k, _way))
    for _fam, (_m, _n, _k) in (("bgemm", BGEMM_SHAPE), ("bgemm_tail", BGEMM_TAIL_SHAPE)):
        _register(_fam, f"{_m}x{_n}x{_k}-{_way}", dict(m=_m, n=_n, k=_k, way=_way, batch=BGEMM_BATCH),
                  functools.partial(gemm_launches, _m, _n, _k, _way, BGEMM_BATCH))
for _s in WGRAD_SHAPES:
    for _way in ("sparse_dy", "sparse_x"):
        _register("wgrad", f"{_shape_id(_s)}-{_way}", dict(shape=_s, way=_way), functools.partial(wgrad_launches, *_s, _way))
for _s in WWINO_SHAPES:
    for _way in ("dy_pixel", "x_pixel"):
        _register("wwino", f"{_shape_id(_s)}-{_way}", dict(shape=_s, way=_way),
                  functools.partial(wwino_launches, _s[0], _s[1] + _s[2], _s[3], _s[4], _s[5], _way))


def case_ids(*families):
    return [k for k, v in CASES.items() if not families or v[0] in families]


@functools.lru_cache(maxsize=4)
def case(key):
    family, name, params, builder = CASES[key]
    return Case(family, name, params, builder())


# ---- reading a mismatch --------------------------------------------------------------------------------------------------
def explain(tag, y, launch, products=PRODUCTS, limit=4):
    """None when ``y`` (fp64, the model's layout) equals the model bit for bit; otherwise the message of the failure: how
    many elements are wrong, and for the first few their coordinates and which limb product is missing, doubled or extra
    there (by comparison with the drop= / double= models)."""
    prods = launch.prods()
    want = sum_products(prods, products)
    bad = ~(y == want)
    if not bool(bad.any()):
        return None
    alt = {}
    for p in PRODUCTS:
        if p in products:
            alt[f"{p} missing"] = sum_products(prods, products, drop=p)
            alt[f"{p} doubled"] = sum_products(prods, products, double=p)
        else:
            alt[f"{p} present (not in this arithmetic)"] = want + prods[p]
    idx = bad.nonzero()
    lines = [f"{tag}: {len(idx)} of {y.numel()} elements differ from the limb model (class {launch.cls}: "
             f"{', '.join(CLASS_LIT[launch.cls])} lit)"]
    for i in idx[:limit]:
        i = tuple(int(v) for v in i)
        why = [k for k, t in alt.items() if prods[k.split(" ")[0]][i] != 0 and y[i] == t[i]]
        lines.append(f"  at {i}: got {float(y[i])!r}, want {float(want[i])!r}: " + ("; ".join(why) or "no single limb product explains it"))
    return "\n".join(lines)


# ---- dense inputs: error statistics ----------------------------------------------------------------------------------------
def rel_l2_stats(y, ref, band=16):
    """(whole tensor, per column [cols], per band of ``band`` rows [bands]) rel-L2 of 2-D ``y`` against ``ref``, fp64."""
    y, ref = y.double().reshape(-1, y.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    d2, r2 = (y - ref) ** 2, ref ** 2
    nb = -(-y.shape[0] // band)
    pad = nb * band - y.shape[0]
    bd = F.pad(d2, (0, 0, 0, pad)).reshape(nb, -1).sum(1)
    br = F.pad(r2, (0, 0, 0, pad)).reshape(nb, -1).sum(1)
    return (d2.sum() / r2.sum()).sqrt().item(), (d2.sum(0) / r2.sum(0)).sqrt(), (bd / br).sqrt()
