"""The fp64 (and fp32) device math, call by call, against extended-precision references on the GPU.

tests/test_fast64.py pins csrc/fast64.hpp compiled for the HOST, where v_rsq_f64 is emulated, the inline assembly is
plain C++ and contraction is off.  Here tests/device_math_check.hip runs the shipped building blocks as the kernels
compile them (the library's own flags) on crafted Philox words — the inputs a random stream reaches with probability
~2^-37 each: the uniforms next to u = 1, u = 2^-53, every table-chunk and table-arc boundary — and holds them to the
bounds of tests/fast64_bounds.py.  The references are numpy long double (64-bit mantissa), the errors those of
tests/host_fast64_check.cpp.  The measured maxima are recorded as junit properties (record_property).

The barrier test: PathState<double>::below_barrier decides from q = fma(P, kExpScale, kq) and hands over to the exact
test B > value() only when |q| <= win_delta.  Paths whose step remainders all sit at +-0.499 drive P - 1 - ln P to ~90 %
of that band; the barrier is placed so that q lands just outside (cheap branch, whole wavefront sure), just inside and
at 0, and every step's count increment must equal B > value()."""
import importlib
import math

import numpy as np
import pytest

import device_math_harness as dmh
import fast64_bounds as bd

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LD = np.longdouble
PI = LD("3.14159265358979323846264338327950288")
SQ2 = np.sqrt(LD(2))
LN2 = LD("0.693147180559945309417232121458176568")
KEXP = 65536.0 / math.log(2.0)          # kExpScale to double precision: only used to place targets, never to check
RNG_SEED = 20261016


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    assert np.finfo(np.longdouble).nmant >= 63, "the references need an x87 long double"
    importlib.import_module("monte-carlo-project-cuda_amd")
    torch.cuda.set_device(0)
    return dmh.load(dmh.compile_harness(tmp_path_factory.mktemp("dm")))


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def out(n, dtype=torch.float64):
    return torch.empty(int(n), dtype=dtype, device="cuda")


def host(t):
    return t.cpu().numpy()


def ulp_err(got, want):
    """|got - want| in ulps of want (fp64 ulp: 2^(e - 53), e the binary exponent of want); want != 0."""
    _, e = np.frexp(want.astype(np.float64))
    return np.abs(got.astype(LD) - want) / np.ldexp(LD(1), e - 53)


def words53(v):
    """(x, y) with x ^ (y << 21) == v, v < 2^53: the two Philox words rocRAND builds a 53-bit uniform from."""
    v = np.asarray(v, dtype=np.uint64)
    y = (v >> np.uint64(21)) & np.uint64(0xFFFFFFFF)
    x = (v & np.uint64(0xFFFFFFFF)) ^ ((y << np.uint64(21)) & np.uint64(0xFFFFFFFF))
    return x.astype(np.uint32), y.astype(np.uint32)


def v53(x, y):
    return x.astype(np.uint64) ^ (y.astype(np.uint64) << np.uint64(21))


def radius_edge_v():
    """v (u = (v + 1) 2^-53) at the radius' edges: the top 65 536 uniforms, u = j 2^-53 for j <= 1024, the grid
    neighbours of every power of two, every table-chunk boundary of neg2log (+- 3 grid steps) reachable by the grid."""
    top = (1 << 53) - 1 - np.arange(65536, dtype=np.uint64)
    small = np.arange(1024, dtype=np.uint64)
    p2 = np.array([(1 << (53 - e)) + d - 1 for e in range(0, 54) for d in range(-4, 5)
                   if 1 <= (1 << (53 - e)) + d <= (1 << 53)], dtype=np.uint64)
    # the chunk index is (hi32(u) - 0x3fe60000) >> 11: boundaries at hi32 = 0x3fe60000 + m 0x800 (low word 0); u is on
    # the grid from 2^-44 up, where its 43 low mantissa bits are zero
    hi = np.arange(0x3D300000, 0x3FF00001, 0x800, dtype=np.uint64)
    u = (hi << np.uint64(32)).view(np.float64)
    base = (u[(u >= 2.0 ** -44) & (u <= 1.0)] * 2.0 ** 53).astype(np.int64)      # v + 1, exact
    chunk = np.concatenate([base + d - 1 for d in range(-3, 4)])
    chunk = chunk[(chunk >= 0) & (chunk < (1 << 53))].astype(np.uint64)
    return np.unique(np.concatenate([top, small, p2, chunk]))


def angle_edge_v():
    """v2 (t = (v2 + 1) 2^-52) at the angle's edges: each of the 512 arcs with the low 44 bits at 0, 2^43 - 1, 2^43,
    2^44 - 1, and t = 2^-52 and t = 2."""
    lows = np.array([0, (1 << 43) - 1, 1 << 43, (1 << 44) - 1], dtype=np.uint64)
    arcs = np.arange(512, dtype=np.uint64) << np.uint64(44)
    v = (arcs[:, None] | lows[None, :]).ravel()
    return np.unique(np.concatenate([v, np.array([0, (1 << 53) - 1], dtype=np.uint64)]))


def random_words(n, k=2, seed=RNG_SEED):
    r = np.random.default_rng(seed)
    return [r.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) for _ in range(k)]


# ---- 1. the uniform --------------------------------------------------------------------------------------------------

def test_uniform_is_exact(L, record_property):
    v = [np.array([0, (1 << 53) - 1], dtype=np.uint64)]
    for e in range(54):
        v.append(np.array([(1 << e) + d for d in (-1, 0, 1) if 0 <= (1 << e) + d < (1 << 53)], dtype=np.uint64))
    x, y = words53(np.concatenate(v))
    rx, ry = random_words(1 << 20, seed=RNG_SEED + 1)
    x, y = np.concatenate([x, rx]), np.concatenate([y, ry])
    n = x.size
    u, a, su, ss = out(n), out(n), out(n), out(n)
    assert L.dm_radius(n, dev(x).data_ptr(), dev(y).data_ptr(), dev(np.ones(n)).data_ptr(),
                       u.data_ptr(), a.data_ptr(), su.data_ptr(), ss.data_ptr()) == 0
    want = (v53(x, y) + np.uint64(1)).astype(np.float64) * 2.0 ** -53       # (v + 1) 2^-53, exact
    bad = np.flatnonzero(host(u) != want)
    record_property("uniform_mismatch", int(bad.size))
    assert bad.size == 0, (x[bad[:4]], y[bad[:4]])


# ---- 2. the radius ---------------------------------------------------------------------------------------------------

def test_radius_neg2log_and_sqrt(L, record_property):
    v = radius_edge_v()
    ex, ey = words53(v)
    rx, ry = random_words(1 << 21, seed=RNG_SEED + 2)
    x, y = np.concatenate([ex, rx]), np.concatenate([ey, ry])
    n = x.size
    ks = np.array([1.0, 0.0126, 3.3e-3, 0.0126 * 1024, 1191.2, 94548.0 * 0.02])
    k = ks[np.arange(n) % ks.size]
    u, a, su, ss = out(n), out(n), out(n), out(n)
    assert L.dm_radius(n, dev(x).data_ptr(), dev(y).data_ptr(), dev(k).data_ptr(),
                       u.data_ptr(), a.data_ptr(), su.data_ptr(), ss.data_ptr()) == 0
    u, a, su, ss = host(u), host(a), host(su), host(ss)
    assert np.array_equal(u, (v53(x, y) + np.uint64(1)).astype(np.float64) * 2.0 ** -53)
    # -2 ln u > 0 for every u in (0, 1]: the radius' v_rsq_f64 seed must stay finite (u = 1 included)
    nonpos = np.flatnonzero(~(a > 0))
    assert nonpos.size == 0, (u[nonpos[:4]], a[nonpos[:4]])
    one = u == 1.0
    assert one.any() and np.all(np.abs(a[one]) <= 1e-15)
    want = -2 * np.log(u[~one].astype(LD))
    e_log = ulp_err(a[~one], want).max()
    a_l = a.astype(LD)
    e_su = ulp_err(su, np.sqrt(a_l)).max()
    e_ss = ulp_err(ss, k.astype(LD) * np.sqrt(a_l)).max()
    assert np.all(np.isfinite(su)) and np.all(np.isfinite(ss))
    record_property("neg2log_ulp", float(e_log))
    record_property("sqrt_unclamped_ulp", float(e_su))
    record_property("sqrt_scaled_ulp", float(e_ss))
    assert e_log <= bd.NEG2LOG_ULP
    assert e_su <= bd.SQRT_UNCLAMPED_ULP
    assert e_ss <= bd.SQRT_SCALED_ULP


# ---- 3. the angle ----------------------------------------------------------------------------------------------------

def angle_words():
    ez, ew = words53(angle_edge_v())
    rz, rw = random_words(1 << 21, seed=RNG_SEED + 3)
    return np.concatenate([ez, rz]), np.concatenate([ew, rw])


def angle_of(z, w):
    t = (v53(z, w) + np.uint64(1)).astype(np.float64) * 2.0 ** -52       # rocRAND's angle uniform, exact
    return PI * t.astype(LD)


def test_angle_plain_table(L, record_property):
    z, w = angle_words()
    n = z.size
    s, c = out(n), out(n)
    assert L.dm_sincos(n, dev(z).data_ptr(), dev(w).data_ptr(), s.data_ptr(), c.data_ptr()) == 0
    ang = angle_of(z, w)
    es = np.abs(host(s).astype(LD) - np.sin(ang)).max()
    ec = np.abs(host(c).astype(LD) - np.cos(ang)).max()
    record_property("sin_abs", float(es))
    record_property("cos_abs", float(ec))
    assert es <= bd.SINCOS_ABS and ec <= bd.SINCOS_ABS


def test_angle_rotated_table(L, record_property):
    # the table MathCtx<double>::init<true>() copies rotated by N/8, as the pair-sum loop reads it
    z, w = angle_words()
    n = z.size
    s, c, s1 = out(n), out(n), out(n)
    assert L.dm_rotated(n, dev(z).data_ptr(), dev(w).data_ptr(), s.data_ptr(), c.data_ptr(), s1.data_ptr()) == 0
    ang = angle_of(z, w) + PI / 4
    s, c = host(s), host(c)
    assert np.array_equal(s, host(s1))                 # sin_bits_rotated<false> is the same sine
    es = np.abs(s.astype(LD) - np.sin(ang)).max()
    ec = np.abs(c.astype(LD) - np.cos(ang)).max()
    record_property("sin_rotated_abs", float(es))
    record_property("cos_rotated_abs", float(ec))
    assert es <= bd.SINCOS_ABS and ec <= bd.SINCOS_ABS


# ---- 4. whole pairs --------------------------------------------------------------------------------------------------

def pair_words():
    """U4 words: random blocks, the radius edges with random angles, the angle edges with random radii."""
    rx, ry, rz, rw = random_words(1 << 21, k=4, seed=RNG_SEED + 4)
    ex, ey = words53(radius_edge_v())
    az, aw = words53(angle_edge_v())
    fx, fy, fz, fw = random_words(ex.size + az.size, k=4, seed=RNG_SEED + 5)
    x = np.concatenate([rx, ex, fx[ex.size:]])
    y = np.concatenate([ry, ey, fy[ex.size:]])
    z = np.concatenate([rz, fz[:ex.size], az])
    w = np.concatenate([rw, fw[:ex.size], aw])
    return np.stack([x, y, z, w], axis=1).astype(np.uint32)


def test_pairs_f64(L, record_property):
    W = pair_words()
    n = W.shape[0]
    z0, z1, ps, hd = out(n), out(n), out(n), out(n)
    d = dev(W.ravel())
    assert L.dm_box_muller64(n, d.data_ptr(), z0.data_ptr(), z1.data_ptr()) == 0
    assert L.dm_pairsum64(n, d.data_ptr(), ps.data_ptr(), hd.data_ptr()) == 0
    u = (v53(W[:, 0], W[:, 1]) + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    r = np.sqrt(-2 * np.log(u.astype(LD)))
    ang = angle_of(W[:, 2], W[:, 3])
    sn, cs = np.sin(ang), np.cos(ang)
    got = {"z0": (host(z0), r * sn), "z1": (host(z1), r * cs),
           "pair_sum": (host(ps) * SQ2, r * (sn + cs)),      # PairSum<double>: units of kUnit = sqrt 2
           "head": (host(hd) * SQ2, r * sn)}                 # head (n == 1): z0 alone
    # u = 1 exactly (probability 2^-53): the table entry that serves it is biased so that -2 ln u = 4e-18 > 0 and the
    # rsq seed stays finite (fast64.hpp sqrt_scaled), so the radius is 2e-9 there instead of 0
    one = u == 1.0
    assert one.sum() >= 1
    err = {}
    for k_, (g, want) in got.items():
        assert np.all(np.isfinite(g)), k_
        assert np.all(np.abs(g[one]) <= 3e-9), (k_, g[one])
        err[k_ + "_rel"] = float((np.abs(g[~one].astype(LD) - want[~one]) / (1 + r[~one])).max())
        record_property(k_ + "_rel", err[k_ + "_rel"])
    assert max(err.values()) <= bd.PAIR_SUM_REL, err


def test_pairs_f32(L, record_property):
    rx, ry, rz, rw = random_words(1 << 20, k=4, seed=RNG_SEED + 6)
    ext = np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    g = np.array(np.meshgrid(ext, ext, ext, ext, indexing="ij")).reshape(4, -1)
    W = np.concatenate([g.T, np.stack([rx, ry, rz, rw], axis=1)]).astype(np.uint32)
    n = W.shape[0]
    o = out(9 * n, torch.float32)
    assert L.dm_f32(n, dev(W.ravel()).data_ptr(), o.data_ptr()) == 0
    o = host(o).reshape(n, 9)
    assert not np.isnan(o).any()

    def uni(words, shift=0.0):   # rocRAND's fp32 uniform fma(float(x), 2^-32, 2^-32 + shift), one rounding
        c = np.float64(np.float32(np.float32(2.0 ** -32) + np.float32(shift)))
        return np.float32(words.astype(np.float32).astype(np.float64) * 2.0 ** -32 + c)

    u0, a0 = uni(W[:, 0]), uni(W[:, 1])
    u1, a1 = uni(W[:, 2]), uni(W[:, 3])
    r0 = np.sqrt(-2 * np.log(u0.astype(LD)))
    r1 = np.sqrt(-2 * np.log(u1.astype(LD)))
    n0, n1 = r0 * np.sin(2 * PI * a0.astype(LD)), r0 * np.cos(2 * PI * a0.astype(LD))
    n2 = r1 * np.sin(2 * PI * a1.astype(LD))
    unit = np.sqrt(4 * LN2)                               # PairSum<float>::kUnit
    err = {
        "f32_z0_abs": np.abs(o[:, 0].astype(LD) - n0).max(),
        "f32_z1_abs": np.abs(o[:, 1].astype(LD) - n1).max(),
        "f32_pair_abs_per_normal": np.abs(o[:, 2].astype(LD) * unit - (n0 + n1)).max() / 2,
        "f32_polar_t_abs": np.abs(o[:, 3].astype(LD) * np.sqrt(2 * LN2) - r0).max(),
        "f32_head1_abs": np.abs(o[:, 7].astype(LD) * unit - n0).max(),
        "f32_head3_abs_per_normal": np.abs(o[:, 8].astype(LD) * unit - (n0 + n1 + n2)).max() / 3,
    }
    for k_, v_ in err.items():
        record_property(k_, float(v_))
    assert max(err.values()) <= bd.F32_NORMAL_ABS, err
    assert np.array_equal(o[:, 4], a0) and np.array_equal(o[:, 6], uni(W[:, 1], 0.125))   # the angles, bit for bit
    assert np.array_equal(o[:, 3], o[:, 5])
    # x = 0: u = 2^-32, the largest radius; x = 0xFFFFFFFF: u = 1, the normals are +-0
    top = W[:, 0] == 0xFFFFFFFF
    assert np.all(o[top][:, [0, 1, 2, 3, 7]] == 0)
    assert np.abs(o[W[:, 0] == 0][:, 3] * math.sqrt(2 * math.log(2)) - math.sqrt(64 * math.log(2))).max() < 4e-6


# ---- 5. exponentials -------------------------------------------------------------------------------------------------

def test_mul_exp_and_exp_of_logreturn(L, record_property):
    r = np.random.default_rng(RNG_SEED + 7)
    n = 1 << 20
    S = 37.0 + r.random(n) * 200.0
    x = np.where(np.arange(n) % 2 == 0, r.uniform(-1, 1, n), r.uniform(-300, 300, n))
    y = r.uniform(-1, 1, n) * KEXP
    xs = np.concatenate([x, [800.0, -800.0]])
    S = np.concatenate([S, [1.0, 1.0]])
    y = np.concatenate([y, [0.0, 0.0]])
    m = xs.size
    me, el = out(m), out(m)
    assert L.dm_exp(m, dev(S).data_ptr(), dev(xs).data_ptr(), dev(y).data_ptr(), me.data_ptr(), el.data_ptr()) == 0
    me, el = host(me), host(el)
    assert np.isinf(me[-2]) and me[-2] > 0 and me[-1] == 0.0      # saturation, never a wrapped finite value
    me, el, S, xs, y = me[:n], el[:n], S[:n], xs[:n], y[:n]
    e = ulp_err(me, S.astype(LD) * np.exp(xs.astype(LD)))
    small = np.abs(xs) <= 1
    e_small = float(e[small].max())
    e_wide = float((e[~small] / np.abs(xs[~small]).astype(LD)).max())
    e_el = float(ulp_err(el, S.astype(LD) * np.exp2(y.astype(LD) / 65536)).max())
    record_property("mul_exp_ulp", e_small)
    record_property("mul_exp_wide_ulp_per_unit_x", e_wide)
    record_property("exp_of_logreturn_ulp", e_el)
    assert e_small <= bd.MUL_EXP_ULP and e_el <= bd.MUL_EXP_ULP
    assert e_wide <= bd.MUL_EXP_WIDE_ULP_PER_UNIT_X


def run_path(L, y_tab, lane_pat, S):
    lanes, n_steps = lane_pat.size, y_tab.shape[1]
    v, k, P = out(lanes * n_steps), out(lanes * n_steps, torch.int32), out(lanes * n_steps)
    assert L.dm_path(lanes, n_steps, dev(y_tab.ravel()).data_ptr(), dev(lane_pat.astype(np.uint32)).data_ptr(),
                     dev(S).data_ptr(), v.data_ptr(), k.data_ptr(), P.data_ptr()) == 0
    return (host(v).reshape(lanes, n_steps), host(k).reshape(lanes, n_steps), host(P).reshape(lanes, n_steps))


def test_path_product_every_step(L, record_property):
    # the GBM recurrence, 252 factors of the benchmark's size: every step's value() against S 2^(sum y / 65536)
    r = np.random.default_rng(RNG_SEED + 8)
    lanes, n_steps = 256, 252
    y_tab = (r.uniform(-1, 1, (lanes, n_steps)) * 0.06 + 1.5e-4) * KEXP
    S = 37.0 + r.random(lanes) * 200.0
    v, k, P = run_path(L, y_tab, np.arange(lanes), S)
    want = S[:, None].astype(LD) * np.exp2(np.cumsum(y_tab.astype(LD), axis=1) / 65536)
    e = float(ulp_err(v, want).max())
    record_property("product252_ulp", e)
    assert e <= bd.PRODUCT252_ULP
    assert np.array_equal(k, np.cumsum(np.rint(y_tab), axis=1).astype(np.int32))   # the exponent is exact


def test_path_product_saturates(L, record_property):
    # running products past DBL_MAX and down through the subnormals: inf, 0 or a subnormal near the reference's grid
    n_steps = 150
    steps = np.array([8 * 65536 + 0.37, -(8 * 65536 + 0.37), 7.9 * 65536, -7.9 * 65536])
    y_tab = np.repeat(steps[:, None], n_steps, axis=1)
    lanes = 64
    pat = np.arange(lanes) % steps.size
    S = 1.0 + np.arange(lanes) / 64.0
    v, _, _ = run_path(L, y_tab, pat, S)
    want = S[:, None].astype(LD) * np.exp2(np.cumsum(y_tab[pat].astype(LD), axis=1) / 65536)
    assert not np.isnan(v).any()
    big = want >= LD(2) ** 1024 * (1 + LD(2) ** -40)
    assert np.all(np.isposinf(v[big])) and big.any()
    normal = (want >= LD(2) ** -1022) & (want < LD(2) ** 1024 * (1 - LD(2) ** -40))
    assert np.all(np.isfinite(v[normal])) and ulp_err(v[normal], want[normal]).max() <= bd.PRODUCT252_ULP
    sub = want < LD(2) ** -1022
    assert sub.any() and np.all(v[sub] >= 0)
    _, e = np.frexp(want[sub].astype(np.float64).clip(min=np.finfo(np.float64).tiny))
    # relative error of the normal product, and the one rounding of ldexp onto the subnormal grid
    tol = bd.PRODUCT252_ULP * np.ldexp(LD(1), e - 53) + LD(2) ** -1074
    dev_ = np.abs(v[sub].astype(LD) - want[sub])
    record_property("subnormal_grid_units", float((dev_ / LD(2) ** -1074).max()))
    assert np.all(dev_ <= tol)
    assert np.any(v[sub] == 0) and np.any((v[sub] > 0) & (v[sub] < 2.0 ** -1022))


# ---- 6. the barrier band ---------------------------------------------------------------------------------------------

BAND_STEPS = [1, 2, 64, 252, 1000, 5001, 30000, 56000, 57000]


def band_patterns(n):
    """Four step sequences whose remainders rr = y - rint(y) all sit at +0.499 or all at -0.499, with rint(y) 0, or
    alternating +3 / -3 (k stays within [-3, 3]): P - 1 - ln P grows as fast as a path of n factors allows."""
    alt = np.where(np.arange(n) % 2 == 0, 3.0, -3.0)
    return np.stack([np.full(n, 0.499), np.full(n, -0.499), alt + 0.499, alt - 0.499])


def band_cases(wd):
    """Target q / win_delta at the last step for two wavefronts: the first all just outside the band (every lane sure:
    the cheap branch), the second just inside and at 0.  Lane l runs pattern l % 4."""
    lane = np.arange(128)
    outside = np.where((lane // 4) % 2 == 0, 1.0, -1.0) * (1 + 1e-3 * (1 + (lane // 8 % 8) / 8.0))
    inside = np.array([1 - 1e-3, -(1 - 1e-3), 0.0, 0.5])[(lane // 4) % 4]
    return np.where(lane < 64, outside, inside) * wd


@pytest.mark.parametrize("restart", [False, True], ids=["start", "restart"])
@pytest.mark.parametrize("n", BAND_STEPS)
def test_barrier_band(L, n, restart, record_property):
    pats = band_patterns(n)
    lane = np.arange(128)
    pat = lane % 4
    # probe: (k, P) at the last step, for each pattern (independent of the start price)
    _, k, P = run_path(L, pats, np.arange(64) % 4, np.ones(64))
    kt, Pt = k[:4, -1].astype(LD), P[:4, -1].astype(LD)
    q0 = kt + (Pt - 1) * LD(KEXP)              # q at the last step when theta = 0
    wd_shipped = dmh.consts(L, n, 100.0, 100.0)[1]
    wd = wd_shipped if math.isfinite(wd_shipped) else dmh.consts(L, 56000, 100.0, 100.0)[1]
    theta = q0[pat] - LD(1) * band_cases(wd).astype(LD)
    S_start = np.full(128, 100.0)
    St0 = 100.0 * (0.9 + 0.2 * lane / 128.0)
    S_from = St0 if restart else S_start
    B = (S_from.astype(LD) * np.exp(theta / LD(KEXP))).astype(np.float64)
    flags, q = out(128 * n, torch.uint8), out(128 * n, torch.float32)
    assert L.dm_barrier(128, n, B.ctypes.data, S_start.ctypes.data, dev(pats.ravel()).data_ptr(),
                        dev(pat.astype(np.uint32)).data_ptr(), dev(St0).data_ptr(), int(restart),
                        flags.data_ptr(), q.data_ptr()) == 0
    f = host(flags).reshape(128, n)
    q = host(q).reshape(128, n).astype(np.float64)
    cheap, exact, sure = f & 1, (f >> 1) & 1, (f >> 2) & 1
    # the contract: the count grows by B > value() at every step of every lane
    bad = np.argwhere(cheap != exact)
    assert bad.size == 0, ("cheap and exact barrier decisions differ", n, restart, bad[:5], q[tuple(bad[0])] / wd)
    # how much of the band the worst remainder pattern uses at the last step (the probe's own P, in long double)
    used = float(((Pt - 1 - np.log(Pt)) * LD(KEXP)).max() / LD(wd))
    qt = q[:, -1] / wd
    if math.isfinite(wd_shipped):
        record_property("band_used", used)
        # the targets were hit: the first wavefront just outside, the second inside and at 0
        assert np.all((np.abs(qt[:64]) > 1 + 5e-4) & (np.abs(qt[:64]) < 1 + 3e-3)), qt[:64]
        assert np.all(np.abs(qt[64:]) < 1 - 5e-4)
        assert np.abs(qt[64:][(lane[64:] // 4) % 4 == 2]).max() * wd < 1e-9
        # the first wavefront took the cheap branch at the last step, the second the exact one
        assert np.all(sure[:64, -1] == 1) and np.all(sure[64:, -1] == 0)
        # and the cheap branch's decision there is the one whose margin is tightest (q just above the band, price
        # just above the barrier by less than the band's error)
        assert np.all(exact[:64, -1] == (qt[:64] < 0))
        if n >= 64:
            assert used > 0.7
    else:
        # no bound beyond L = 0.3: every step of every wavefront takes the exact test
        assert not sure.any()
