"""Nets on which every forward path of every operand format must equal the float64 result bit for bit ("exact-arithmetic nets").

DESIGN 3.2: every contraction is hi*hi + lo*hi + hi*lo on f16 parts (hi = f16(x), lo = f16(x - hi)) in an fp32 accumulator; the rest is fp32 bias adds, LeakyReLU and
depthwise sums.  If (1) every product the kernels form is exact and the one they leave out (lo*lo) is zero, (2) every partial sum, in any order, is an integer below 2^24 of
one unit (a power of two), and (3) every pre-activation is >= 0 (the slope 0.2 never multiplies anything), then whatever the summation order, split-K plan, tile order or
cache state the result is the float64 one.  `make` builds such nets, `prove` shows (1)-(3) for EVERY board by interval propagation and says which net modes are exact,
`forward64` is the float64 reference.  Plain numpy; nothing here needs a GPU.

Families:
  narrow       every weight f16-exact, every trunk activation and the trunk output <= 2047 units: every lo of a product whose OTHER factor has one is zero (h0 and h1
               carry 16..19 bits, against f16-exact weights).  Exact in every mode.
  wide_act     the trunk output carries up to ~13 bits (non-zero lo in fc0's operand rows and difference rows), all weights f16-exact.  Exact where fc0's correction terms
               are f16 or the kernels are fp32; not with fp6 correction terms (fp6 / mixed / the default mode, which may choose either).
  wide_weight  ONE matrix (`wide=`, a tensor index of WIDE_WEIGHT_TENSORS: one trunk 1x1 per block -- block 0's down-projection, block 1's pointwise, block 2's
               up-projection --, 23 fc0, 25 fc1, 29 policy head) carries 12 significant bits (non-zero lo fragments) while its input is <= 11 bits.  Long trunk weights
               give every later trunk activation, the base entries and fc0's operand rows a non-zero lo (~22 bits).  Long trunk or fc0 weights: fp32 kernels and the
               f16 format only.
"""
import numpy as np

C, M, F = 128, 32, 512
FAMILIES = ("narrow", "wide_act", "wide_weight")
MODES = ("f32", "fp6", "f16", "mixed", "default")  # OMOK_NET_F32, _F16X3_FP6, _F16X3_F16, _F16X3_MIXED, OMOK_NET_F16X3
F16_MAX = 65504.0
BIASES = (1, 24, 26, 28, 30) + tuple(2 + 7 * b + o for b in range(3) for o in (1, 4, 6))
TRUNK_WIDE = (2, 12, 21)  # one trunk 1x1 per block: block 0's down-projection, block 1's pointwise, block 2's up-projection
WIDE_WEIGHT_TENSORS = TRUNK_WIDE + (23, 25, 29)  # ... fc0, fc1 and the policy head


def tensor_shapes(n):
    hw = n * n
    shapes = [(1, 1, 3, C), (C,)]
    for _ in range(3):
        shapes += [(1, 1, C, M), (M,), (3, 3, M, 1), (1, 1, M, M), (M,), (1, 1, M, C), (C,)]
    return shapes + [(C * hw, F), (F,), (F, F), (F,), (F, 1), (1,), (F, hw), (hw,)]


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# units and bit counts
def unit_of(a):
    """the largest power of two of which every entry of `a` is an integer multiple (1.0 for an all-zero array)"""
    v = np.abs(np.asarray(a, dtype=np.float64).ravel())
    v = v[v != 0]
    if v.size == 0:
        return 1.0
    m, e = np.frexp(v)  # v = m 2^e, m in [0.5, 1): the integer m 2^53 has 53 - tz significant bits
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = mi & -mi  # lowest set bit
    tz = np.round(np.log2(low.astype(np.float64))).astype(np.int64)
    return float(2.0 ** int((e - 53 + tz).min()))


def sig_bits(a):
    """the largest number of significant bits (top set bit .. lowest set bit) of an entry of `a`"""
    v = np.abs(np.asarray(a, dtype=np.float64).ravel())
    v = v[v != 0]
    if v.size == 0:
        return 0
    m, _ = np.frexp(v)
    mi = (m * 2.0 ** 53).astype(np.int64)
    tz = np.round(np.log2((mi & -mi).astype(np.float64))).astype(np.int64)
    return int((53 - tz).max())


def _bits(x):
    """bits of the integer bound x (0 -> 0)"""
    return int(np.ceil(np.log2(float(x) + 1.0))) if x > 0 else 0


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# builder
def _cover(rng, rows, cols, nz):
    """row indices [cols][nz]: concatenated permutations of the rows dealt to the columns, so every row is picked before any is picked twice more often"""
    need = cols * nz
    seq = np.concatenate([rng.permutation(rows) for _ in range(-(-need // rows))])[:need]
    return seq.reshape(cols, nz)


def _sparse(rng, rows, cols, nz, values, scale, signed=False, p=None):
    w = np.zeros((rows, cols), dtype=np.float64)
    idx = _cover(rng, rows, cols, nz)
    val = rng.choice(values, size=idx.shape, p=p).astype(np.float64)
    if signed:
        val *= rng.choice([-1.0, 1.0], size=idx.shape)
    w[idx, np.arange(cols)[:, None]] = val * scale
    return w


def _trunk_bounds(t):
    """per-channel upper bounds of the trunk output over all boards: inputs in [0, 1], weights and biases >= 0 (asserted by prove)"""
    ub = np.abs(t[0].reshape(3, C)).sum(0) + np.abs(t[1])
    for b in range(3):
        w0, b0, dw, pw, b1, w2, b2 = t[2 + 7 * b: 9 + 7 * b]
        h = ub @ np.abs(w0.reshape(C, M)) + np.abs(b0)
        d = h * np.abs(dw.reshape(9, M)).sum(0)
        g = d @ np.abs(pw.reshape(M, M)) + np.abs(b1)
        ub = g @ np.abs(w2.reshape(M, C)) + np.abs(b2) + ub
    return ub


def make(n, seed, family="narrow", wide=None):
    """31 float32 tensors in the reference's variable order.  family "wide_weight": `wide` names the tensor that carries the long weights."""
    assert family in FAMILIES and (wide in WIDE_WEIGHT_TENSORS if family == "wide_weight" else wide is None), (family, wide)
    trunk_wide = wide in TRUNK_WIDE
    hw = n * n
    rng = np.random.default_rng([int(seed), n, FAMILIES.index(family), 0 if wide is None else int(wide)])
    t = [None] * 31
    # units of 1/2 the trunk output may reach (prove's own limits: 2047 for a zero lo; 2^22 -- with 12-bit weights in the trunk the unit is 1/8192, which leaves 1023)
    limit = 8191 if family == "wide_act" else 1000 if trunk_wide else 1800
    top = 2 if trunk_wide else 3  # (biases 0..1 halves on the thinner trunk)
    for p2 in (0.1, 0.05, 0.02, 0.0):  # the share of twos among the trunk's ones: the first that keeps the bound (prove has the last word)
        one_two = ([1, 2], [1.0 - p2, p2])
        # conv_in: 1..2 of the 3 input channels per output channel; unit 1/2
        cw = np.zeros((3, C))
        for o in range(C):
            k = rng.choice(3, size=int(rng.integers(1, 3)), replace=False)
            cw[k, o] = rng.choice(one_two[0], size=len(k), p=one_two[1]) * 0.5
        t[0], t[1] = cw, rng.integers(0, top, C) * 0.5
        for b in range(3):
            # scales of the four layers multiply to one: the branch comes back in the stream's unit, with other exponents on the way
            s0, sd, sp, s2 = 2.0 ** -(1 + b), 2.0, 2.0 ** b, 1.0
            q = 2 + 7 * b
            t[q] = _sparse(rng, C, M, 2, *one_two[:1], s0, p=one_two[1])
            u_h = 0.5 * s0
            t[q + 1] = rng.integers(0, top, M) * u_h
            dw = np.zeros((9, M))
            for c in range(M):  # two taps per channel: (c + 3 seed + b) mod 9, so that the seeds cover every tap of every channel group, and a random other one
                own = (c + 3 * int(seed) + b) % 9
                dw[own, c] = sd
                dw[(own + int(rng.integers(1, 9))) % 9, c] = sd
            t[q + 2] = dw
            t[q + 3] = _sparse(rng, M, M, 1, [1], sp)
            t[q + 4] = rng.integers(0, top, M) * (u_h * sd * sp)
            up_vals, up_p = one_two
            if family == "wide_act" and b == 2:
                up_vals, up_p = list(range(1, 25)), None  # the last up-projection spreads the trunk output over ~13 bits
            t[q + 5] = _sparse(rng, M, C, 1, up_vals, s2, p=up_p)
            t[q + 6] = rng.integers(0, top, C) * 0.5
        if trunk_wide:  # the ones (and twos) of that matrix become odd 12-bit integers / 4096 of themselves
            nzm = t[wide] != 0
            t[wide][nzm] *= (2 * rng.integers(1024, 2048, int(nzm.sum())) + 1) / 4096.0
        if _trunk_bounds(t).max() / 0.5 <= limit:
            break
    ub = _trunk_bounds(t)
    u_t = 0.5
    K0 = C * hw
    ub_rows = np.tile(ub / u_t, hw)  # fc0 row = pixel * 128 + channel
    s_fc0, s_fc1 = 2.0 ** -6, 0.25
    long_w = lambda shape: (2 * rng.integers(1024, 2048, shape) + 1) / 4096.0  # odd 12-bit integers / 2^12: hi + a non-zero lo in f16
    if family != "wide_weight":
        # fc0: a column budget of T0 units (trunk unit x weight unit); rows dealt so that every (pixel, channel) is used by some column
        T0 = 2.0 ** (15 if n == 9 else 16) / (8.0 if family == "wide_act" else 1.0)
        m0 = max(8, int(T0 / (2.0 * ub_rows.mean())))
        t[23] = _sparse(rng, K0, F, m0, [1, 2, 3], s_fc0)
        w1 = np.zeros((F, F))
        for _ in range(4):  # four permutations: every h0 column feeds four h1 columns
            w1[rng.permutation(F), np.arange(F)] = rng.choice([1, 2, 3], size=F) * s_fc1
        kp, s_hd = -(-F // hw) + 1, 2.0 ** -7  # every h1 column reaches a logit
        wp = _sparse(rng, F, hw, kp, [1, 2], s_hd, signed=True)
    else:
        # a thin tail leaves the bits for ONE long matrix: fc0 one weight per column on rows bounded by 500 units, fc1 a permutation, one head weight per logit
        small = np.flatnonzero(ub_rows <= 500)
        assert len(small) >= 64, "no trunk channel is small enough for the thin tail"
        w0 = np.zeros((K0, F))
        idx = small[_cover(rng, len(small), F, 1)]
        w0[idx, np.arange(F)[:, None]] = s_fc0 * (long_w(idx.shape) if wide == 23 else 1.0)
        t[23] = w0
        w1 = _sparse(rng, F, F, 1, [1], s_fc1)
        if wide == 25:
            w1[w1 != 0] = s_fc1 * long_w(int((w1 != 0).sum()))
        s_hd = 2.0 ** 4
        wp = _sparse(rng, F, hw, 1, [1, 2], s_hd, signed=True)
        if wide == 29:
            nzm = wp != 0
            wp[nzm] = np.sign(wp[nzm]) * s_hd * long_w(int(nzm.sum()))
    u_h0 = u_t * unit_of(t[23])
    t[24] = rng.integers(0, 4, F) * u_h0
    u_h1 = u_h0 * unit_of(w1)
    t[25], t[26] = w1, rng.integers(0, 4, F) * u_h1
    u_lg = u_h1 * unit_of(wp)
    t[29], t[30] = wp, rng.integers(-3, 4, hw) * u_lg * 4
    s_v = s_hd / (16.0 if family == "wide_weight" else 4.0)
    t[27] = _sparse(rng, F, 1, 6, [1, 2], s_v, signed=True)
    t[28] = np.array([float(rng.integers(-3, 4)) * u_h1 * s_v])
    out = [np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(s)).astype(np.float32) for a, s in zip(t, tensor_shapes(n))]
    for a, b in zip(out, t):
        assert np.array_equal(a.astype(np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()), "a generated weight is not an fp32 value"
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# proof
class NotExact(AssertionError):
    pass


def _need(cond, msg):
    if not cond:
        raise NotExact(msg)


def fc0_summary(n, w23):
    """what prove needs of fc0's matrix: (sum over pixels of |w| [128][512], unit, significant bits, largest magnitude, smallest entry)"""
    w = np.asarray(w23).reshape(n * n, C, F)
    nz = w[w != 0].astype(np.float64)
    return np.abs(w).sum(axis=0, dtype=np.float64), unit_of(nz), sig_bits(nz), float(np.abs(nz).max()) if nz.size else 0.0, float(nz.min()) if nz.size else 0.0


def prove(n, tensors, mode=None, fc0=None):
    """Interval propagation over ALL boards (every input value in [0, 1]: a superset of the six legal (mine, theirs, turn) patterns per cell, whose flat layout puts any
    three of the row's floats into a net pixel), per-channel upper bounds without pixel dependence.  Raises NotExact unless conditions (1)-(3) of the module text hold in
    at least the fp32 kernels or one split format; returns the bounds and `modes`, the subset of MODES in which the net is exact.  With `mode` given: raises unless that
    mode is exact.  `fc0`: a fc0_summary of tensor 23 computed earlier, for callers that prove many nets with one fc0 matrix.

    A contraction a.w of an activation bounded by A units of u_a with a matrix of unit u_w:
      all modes   every partial sum is an integer of u_a u_w below 2^24; the bias add stays below 2^24 of the finer of both units; pre-activation >= 0
      split (f16 terms)   each weight is hi + lo in f16 (<= 22 significant bits, a multiple of 2^-24, below 65504); each activation likewise (A < 2^22, magnitude below
                  65504); the dropped lo*lo is zero: A <= 2047 (activation lo zero) or every weight <= 11 bits (weight lo zero)
      fp6 terms   (fc0 in the fp6 format, and the difference rows of the mixed format) both lo zero: a non-zero fp6 correction term is not exact
      fp32        each product fits fp32 without relying on a fused multiply-add: bits(A) + bits(w) <= 24"""
    hw = n * n
    assert len(tensors) == 31 and all(np.asarray(a).size == int(np.prod(s)) for a, s in zip(tensors, tensor_shapes(n)))
    t = [None if i == 23 else np.asarray(a, dtype=np.float64) for i, a in enumerate(tensors)]
    aw23, u_w23, wb23, max23, min23 = fc0 if fc0 is not None else fc0_summary(n, tensors[23])
    for i in range(27):  # everything up to h1 is non-negative: every pre-activation is >= 0 on every board
        _need((min23 if i == 23 else t[i].min()) >= 0.0, f"tensor {i} has a negative entry: a pre-activation could be negative")
    for i, a in enumerate(t):
        if i in BIASES:  # (biases are added in fp32)
            continue
        bits, top, unit = (wb23, max23, u_w23) if i == 23 else (sig_bits(a), np.abs(a).max(), unit_of(a))
        _need(bits <= 22 and top < F16_MAX and unit >= 2.0 ** -24, f"tensor {i} is not hi + lo in f16")
    split_ok, f32_ok = [True], [True]
    why = {}
    report = {}

    def layer(name, ub_in, u_in, w, bias, split_out=True):
        """bounds of out = in . w + bias; records which kernels are exact on it"""
        aw = np.abs(w)
        u_w, wb = unit_of(w), sig_bits(w)
        a_bits = _bits(ub_in.max() / u_in)
        u_p = u_in * u_w
        dot = ub_in @ aw  # bound of sum |a| |w|: every partial sum of every order is inside it
        _need(dot.max() / u_p < 2.0 ** 24, f"{name}: a partial sum can reach {dot.max() / u_p:.3g} units (2^24 = 16777216)")
        u_out = min(u_p, unit_of(bias)) if np.any(bias != 0) else u_p
        ub = dot + np.abs(bias)
        _need(ub.max() / u_out < 2.0 ** 24, f"{name}: the bias add can reach {ub.max() / u_out:.3g} units")
        if split_out:
            _need(ub.max() / u_out < 2.0 ** 22 and ub.max() < F16_MAX - 32, f"{name}: the output ({ub.max() / u_out:.3g} units, magnitude {ub.max():.3g}) does not split into hi | lo f16")
        if not (ub_in.max() / u_in <= 2047 or wb <= 11):
            split_ok[0] = False
            why.setdefault("split", f"{name}: activation and weight both carry a lo part: the kernels drop lo*lo")
        if a_bits + wb > 24:
            f32_ok[0] = False
            why.setdefault("f32", f"{name}: a product needs {a_bits} + {wb} bits")
        report[name] = {"units": float(ub.max() / u_out), "magnitude": float(ub.max()), "unit": u_out, "in_bits": a_bits, "w_bits": wb}
        return ub, u_out

    ub, u = layer("conv_in", np.ones(3), 1.0, t[0].reshape(3, C), t[1].ravel())
    for b in range(3):
        w0, b0, dw, pw, b1, w2, b2 = t[2 + 7 * b: 9 + 7 * b]
        h, u_h = layer(f"block{b}.down", ub, u, w0.reshape(C, M), b0.ravel())
        taps = dw.reshape(9, M)
        u_d = u_h * unit_of(taps)
        d = h * taps.sum(0)  # fp32 VALU sums of h * tap: each product must fit fp32 on its own
        _need(_bits(h.max() / u_h) + sig_bits(taps) <= 24 and d.max() / u_d < 2.0 ** 22 and d.max() < F16_MAX - 32, f"block{b}.depthwise: {d.max() / u_d:.3g} units")
        report[f"block{b}.depthwise"] = {"units": float(d.max() / u_d), "magnitude": float(d.max()), "unit": u_d}
        g, u_g = layer(f"block{b}.pointwise", d, u_d, pw.reshape(M, M), b1.ravel())
        x, u_x = layer(f"block{b}.up", g, u_g, w2.reshape(M, C), b2.ravel(), split_out=False)
        u_new = min(u, u_x)
        ub = x + ub
        u = u_new
        _need(ub.max() / u < 2.0 ** 22 and ub.max() < F16_MAX - 32, f"block{b}: the residual stream ({ub.max() / u:.3g} units) does not split into hi | lo f16")
        report[f"block{b}.out"] = {"units": float(ub.max() / u), "magnitude": float(ub.max()), "unit": u}
    trunk_units = float(ub.max() / u)
    # fc0 row = pixel * 128 + channel.  Difference rows hold child - base: within +- the same bound, so the same conditions cover them.
    u_w, wb, a_bits = u_w23, wb23, _bits(trunk_units)
    dot = ub @ aw23
    name = "fc0"
    _need(dot.max() / (u * u_w) < 2.0 ** 24, f"fc0: a partial sum can reach {dot.max() / (u * u_w):.3g} units (2^24 = 16777216)")
    u_h0 = min(u * u_w, unit_of(t[24])) if np.any(t[24] != 0) else u * u_w
    h0 = dot + np.abs(t[24].ravel())
    _need(h0.max() / u_h0 < 2.0 ** 22 and h0.max() < F16_MAX - 32, f"fc0: h0 ({h0.max() / u_h0:.3g} units, magnitude {h0.max():.3g}) does not split into hi | lo f16")
    a_narrow, w_narrow = trunk_units <= 2047, wb <= 11
    fc0_f16 = a_narrow or w_narrow
    fc0_fp6 = a_narrow and w_narrow
    if not fc0_f16:
        why["fc0_f16"] = "fc0: activation and weight both carry a lo part"
    if not fc0_fp6:
        why["fc0_fp6"] = f"fc0: {'the trunk output' if not a_narrow else 'the weight'} has a non-zero lo: an fp6 correction term is not exact"
    if a_bits + wb > 24:
        f32_ok[0] = False
        why.setdefault("f32", f"fc0: a product needs {a_bits} + {wb} bits")
    report[name] = {"units": float(h0.max() / u_h0), "magnitude": float(h0.max()), "unit": u_h0, "in_bits": a_bits, "w_bits": wb}
    h1, u_h1 = layer("fc1", h0, u_h0, t[25].reshape(F, F), t[26].ravel())
    lg, u_lg = layer("policy_head", h1, u_h1, t[29].reshape(F, hw), t[30].ravel(), split_out=False)
    vp, u_vp = layer("value_head", h1, u_h1, t[27].reshape(F, 1), t[28].ravel(), split_out=False)
    modes = set()
    if f32_ok[0]:
        modes.add("f32")
    if split_ok[0] and fc0_f16:
        modes.add("f16")
    if split_ok[0] and fc0_fp6:
        modes |= {"fp6", "mixed", "default"}  # (the default mode's probe may keep any of the three formats: all of them must be exact)
    _need(modes, "no net mode is exact on this net: " + "; ".join(why.values()))
    if mode is not None:
        _need(mode in modes, f"mode {mode} is not exact on this net: " + "; ".join(why.values()))
    return {"modes": modes, "why_not": why, "layers": report, "trunk_units": trunk_units, "h0_units": report["fc0"]["units"], "h1_units": report["fc1"]["units"],
            "h0_magnitude": report["fc0"]["magnitude"], "h1_magnitude": report["fc1"]["magnitude"], "logit_bound": report["policy_head"]["magnitude"],
            "vpre_bound": report["value_head"]["magnitude"], "units": {"trunk": u, "h0": u_h0, "h1": u_h1, "logit": u_lg, "vpre": u_vp}}


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# float64 reference
class Ref:
    """float64 copies of a net's tensors (fc0 column-compressed: its columns are sparse) and its forward"""

    def __init__(self, n, tensors):
        self.n, self.hw = n, n * n
        self.t = [np.asarray(a, dtype=np.float64).reshape(s) for a, s in zip(tensors, tensor_shapes(n))]
        self.units = None  # (forward64: prove's units, computed once)
        self.refresh_fc0()

    def refresh_fc0(self):
        w = self.t[23]
        cols, rows = np.nonzero(w.T)  # sorted by column
        self.rows, self.vals = rows, w[rows, cols]
        self.indptr = np.searchsorted(cols, np.arange(F + 1))
        self.dense = bool(np.any(np.diff(self.indptr) == 0)) or len(rows) > w.size // 8  # (reduceat needs non-empty columns)
        try:  # (faster where scipy is installed; float64 sums of integers below 2^53 do not depend on the order)
            from scipy import sparse
            self.csc = sparse.csc_matrix((self.vals, rows, self.indptr), shape=w.shape)
        except ImportError:
            self.csc = None

    def trunk(self, x):
        n, t = self.n, self.t
        x = np.asarray(x, dtype=np.float64).reshape(-1, 3)  # NHWC view of the flat encoder.rs rows: a net pixel is three consecutive floats
        rows = len(x) // self.hw
        x = self._act(x @ t[0].reshape(3, C) + t[1])
        for b in range(3):
            w0, b0, dw, pw, b1, w2, b2 = t[2 + 7 * b: 9 + 7 * b]
            h = self._act(x @ w0.reshape(C, M) + b0).reshape(rows, n, n, M)
            hp = np.pad(h, ((0, 0), (1, 1), (1, 1), (0, 0)))
            d = np.zeros_like(h)
            for dy in range(3):
                for dx in range(3):
                    if np.any(dw[dy, dx, :, 0] != 0):
                        d += hp[:, dy:dy + n, dx:dx + n, :] * dw[dy, dx, :, 0]
            g = self._act(d.reshape(-1, M) @ pw.reshape(M, M) + b1)
            x = self._act(g @ w2.reshape(M, C) + b2 + x)
        return x.reshape(rows, -1)

    @staticmethod
    def _act(a):
        return np.where(a > 0, a, 0.2 * a)

    def fc0(self, f):
        if self.csc is not None:
            return np.asarray(f @ self.csc)
        if self.dense:
            return f @ self.t[23]
        out = np.empty((len(f), F))
        for s in range(0, len(f), 64):
            out[s:s + 64] = np.add.reduceat(f[s:s + 64][:, self.rows] * self.vals, self.indptr[:-1], axis=1)
        return out

    def tail(self, f):
        t = self.t
        h0 = self._act(self.fc0(f) + t[24])
        h1 = self._act(h0 @ t[25] + t[26])
        return h0, h1, h1 @ t[29] + t[30], (h1 @ t[27] + t[28]).reshape(-1)

    def forward(self, x):
        f = self.trunk(x)
        return (f,) + self.tail(f)


def forward64(n, tensors, x, check=True):
    """(trunk output [B][HW*128] in fc0's row order, h0, h1, logits [B][HW], vpre [B]) in float64.  With `check`: asserts on these rows what `prove` shows for all boards --
    every value is an integer multiple of its unit, converts to float32 without rounding, and no pre-activation was negative."""
    ref = tensors if isinstance(tensors, Ref) else Ref(n, tensors)
    out = ref.forward(x)
    if check:
        if ref.units is None:
            ref.units = prove(n, ref.t)["units"]
        u = ref.units
        for name, a in zip(("trunk", "h0", "h1", "logit", "vpre"), out):
            q = a / u[name]
            assert np.array_equal(q, np.rint(q)), f"{name}: a value is no multiple of its unit {u[name]}"
            assert np.array_equal(a.astype(np.float32).astype(np.float64), a), f"{name}: a value does not convert to float32 exactly"
            if name in ("trunk", "h0", "h1"):
                assert a.min() >= 0.0, f"{name}: negative"
    return out


def softmax_tanh64(logits, vpre):
    """AgentModel::evaluate_pv's outputs from exact logits, in float64"""
    z = logits - logits.max(axis=1, keepdims=True)
    e = np.exp(z)
    return e / e.sum(axis=1, keepdims=True), np.tanh(vpre)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# rows
def plain_rows(n, count=300, seed=5):
    """`count` positions in the encoder.rs layout: the empty board, one stone in a corner / on an edge / in the centre, the full board minus one cell, each with both sides
    to move, then random positions (helpers.random_positions)."""
    from oracle import oracle as O
    from helpers import draw_sequence, random_positions
    hw = n * n
    special = []
    seq = draw_sequence(n)
    for moves in ([], [0], [n - 1], [hw - 1], [n // 2], [hw // 2], seq[:-1], seq[:-2]):
        env = O.Environment(n)
        for c in moves:
            env.place_stone(int(c))
        special += [env.encode_nn_input(O.MODE_PLAYER), env.encode_nn_input(O.MODE_OPPONENT)]
    special = np.stack(special).astype(np.float32)
    return np.concatenate([special, random_positions(n, count - len(special), seed)])


# every (n, seed, family, wide) the GPU tests load: tests/test_exact_nets.py proves each of them
GPU_NETS = [(n, seed, "narrow", None) for n in (9, 15) for seed in (0, 1, 2)] + [(n, 0, "wide_act", None) for n in (9, 15)] + \
    [(n, 0, "wide_weight", w) for n in (9, 15) for w in WIDE_WEIGHT_TENSORS]
EXPECTED_MODES = {"narrow": set(MODES), "wide_act": {"f32", "f16"}, ("wide_weight", 23): {"f32", "f16"}, ("wide_weight", 2): {"f32", "f16"},
                  ("wide_weight", 12): {"f32", "f16"}, ("wide_weight", 21): {"f32", "f16"}, ("wide_weight", 25): set(MODES), ("wide_weight", 29): set(MODES)}


def expected_modes(family, wide=None):
    return EXPECTED_MODES[(family, wide) if wide is not None else family]


def dense_positions(n, games, stones, seed):
    """boards [games][HW] of Stone bytes with `stones` stones each, a stone in every corner: random subsets of the five-free colouring of helpers.draw_sequence (a subset
    of runs of at most four has no run of five), Black one stone ahead when `stones` is odd.  Children of such positions have windows on every edge and corner."""
    from helpers import draw_sequence
    hw = n * n
    seq = draw_sequence(n)
    black, white = np.array(seq[0::2]), np.array(seq[1::2])
    corners = {0, n - 1, hw - n, hw - 1}
    rng = np.random.default_rng([seed, n, stones])
    out = np.zeros((games, hw), dtype=np.uint8)
    for g in range(games):
        for cells, count, stone in ((black, (stones + 1) // 2, 1), (white, stones // 2, 2)):
            must = [c for c in cells if int(c) in corners]
            rest = rng.permutation([c for c in cells if int(c) not in corners])[: count - len(must)]
            out[g, np.concatenate([must, rest]).astype(np.int64)] = stone
    return out
