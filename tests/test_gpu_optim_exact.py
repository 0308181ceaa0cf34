"""The four optimiser kernels (csrc/optim.hip: mt_adam, mt_sumsq, clip_coef, mt_axpby) called through
the C API on hand-built isr_mt_tensor / isr_mt_chunk tables, against tests/optim_ref.py.

AdamOp is explicit fmaf / sqrtf / divide / single fp32 operations, all correctly rounded on the
device with denormals on, so Adam is compared bit for bit (int32 views: the sign of zero counts), and
so are the scale kernel (one multiply), the clip coefficient (one add, one divide), the integer sums of
squares and the EMA wherever its two products are exact.  The only tolerances are derived ones: gamma_n
of the summed squares for mt_sumsq on randn data, one fp32 ulp on the norm of a sum that is no perfect
square (the device's double sqrt), and test_gpu_glue.py's 2^-21 of the summed magnitudes for the EMA
with a general d.

Discipline of every case: all operands of a launch are slices of one fp32 arena filled with SENTINEL;
only the elements of the chunks hold data.  Afterwards the whole arena is compared with the expected
one, so every element outside the chunks (the rest of each tensor, the gaps between tensors) and every
read-only operand must still hold its bits.  LAYOUT is the list of tensors every kernel runs over:
the chunk lengths at which a thread's trip count and the float4 / scalar choice change, chunk starts
that are and are not multiples of four floats, each operand alone off the 16-byte grid, a chunk in
the middle of a tensor, two chunks of one tensor, a tensor split as optim.py splits it, and the
chunk table shuffled so that the tensors' chunks interleave."""
import ctypes
import math

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.0
F32 = np.float32
CHUNK = 65536
LENS = [1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1028, 65536]


@pytest.fixture(scope="module", autouse=True)
def lib(built_lib):
    return built_lib


# ------------------------------------------------------------------ tables
def _spec(n, offs, chunks, kind="rand"):
    assert all(0 <= s and 0 < ln and s + ln <= n for s, ln in chunks)
    return dict(n=n, offs=tuple(offs), chunks=list(chunks), kind=kind)


def _layout():
    al = (0, 0, 0, 0)
    ts = [_spec(n, al, [(0, n)]) for n in LENS]
    for start in (4, 1, 2, 3):  # 4: float4 path; 1, 2, 3 with len % 4 == 0: misaligned start, scalar path
        ts += [_spec(start + ln + 3, al, [(start, ln)]) for ln in (4, 256, 1028)]
    ts.append(_spec(4 + 255 + 1, al, [(4, 255)]))
    for which in range(4):  # p, g, m or v alone one float off the 16-byte grid
        offs = [int(k == which) for k in range(4)]
        ts += [_spec(ln, offs, [(0, ln)]) for ln in (4, 256, 1028)]
    ts.append(_spec(3 + 1024 + 2, (1, 1, 1, 1), [(3, 1024)]))  # every base off by one, start 3: aligned again
    ts.append(_spec(3000, al, [(1000, 1024)]))                 # the middle of a tensor
    ts.append(_spec(4096, al, [(0, 1024), (2048, 1028)]))      # two chunks of one tensor, a gap between
    n = 2 * CHUNK + 5
    ts.append(_spec(n, al, [(s, min(CHUNK, n - s)) for s in range(0, n, CHUNK)]))  # optim._Tables' split
    ts.append(_spec(1028, al, [(0, 1028)], "zero"))    # g = m = v = 0
    ts.append(_spec(1027, al, [(0, 1027)], "gzero"))   # g = +-0, m and v not
    return ts


LAYOUT = _layout()
SMALL = [t for t in LAYOUT if t["n"] <= 4096]


class Tables:
    """An arena, the operand slices of `layout` in it and the device tables over them.  `ops`: which of
    p, g, m, v exist (the others are null pointers, as optim.py passes them).  fill(kind, rng, n) returns
    the fp32 data of each operand in `ops` for n chunk elements."""

    def __init__(self, layout, ops, fill, seed):
        rng = np.random.default_rng(seed)
        top, base = 64, []
        for t in layout:
            row = []
            for k in range(4):
                if "pgmv"[k] not in ops:
                    row.append(None)
                    continue
                i = (top + 3) // 4 * 4 + t["offs"][k]
                top = i + t["n"] + 16
                row.append(i)
            base.append(row)
        self.size = top + 64
        self.init = np.full(self.size, SENTINEL, dtype=F32)
        self.idx = {o: [] for o in ops}  # arena index of every chunk element, chunk after chunk
        self.chunks = []                 # (tensor, start, len) in table order
        for ti, t in enumerate(layout):
            for s, ln in t["chunks"]:
                self.chunks.append((ti, s, ln))
        order = np.random.default_rng(1234).permutation(len(self.chunks))
        self.chunks = [self.chunks[k] for k in order]
        for ti, s, ln in self.chunks:
            data = fill(layout[ti]["kind"], rng, ln)
            for o in ops:
                i = base[ti]["pgmv".index(o)] + s
                assert 64 <= i and i + ln + 16 <= self.size
                self.init[i:i + ln] = data[o]
                self.idx[o].append(np.arange(i, i + ln))
        self.idx = {o: np.concatenate(v) for o, v in self.idx.items()}
        self.bounds = np.cumsum([0] + [c[2] for c in self.chunks])  # chunk k is idx[bounds[k]:bounds[k + 1]]
        self.arena = torch.from_numpy(self.init).to(DEV)
        p0 = self.arena.data_ptr()
        assert p0 % 16 == 0
        rows = [[0 if b is None else p0 + 4 * b for b in row] + [t["n"]] for row, t in zip(base, layout)]
        self.ts = torch.tensor(rows, dtype=torch.int64).to(DEV)
        self.cs = torch.tensor([[ti | (ln << 32), s] for ti, s, ln in self.chunks], dtype=torch.int64).to(DEV)
        self.n = len(self.chunks)

    def args(self):
        return self.ts.data_ptr(), self.cs.data_ptr(), self.n

    def check(self, expected: np.ndarray, what=""):
        """The whole arena, bit for bit."""
        torch.cuda.synchronize()
        got = self.arena.cpu().numpy()
        a, b = got.view(np.int32), expected.view(np.int32)
        if np.array_equal(a, b):
            return
        bad = np.flatnonzero(a != b)
        i = int(bad[0])
        where = "outside every chunk"
        for o, idx in self.idx.items():
            hit = np.flatnonzero(idx == i)
            if hit.size:
                k = int(np.searchsorted(self.bounds, hit[0], side="right")) - 1
                where = (f"operand {o}, chunk {k} (tensor, start, len) = {self.chunks[k]}, "
                         f"element {int(hit[0] - self.bounds[k])}")
        raise AssertionError(f"{what}: {bad.size} of {a.size} arena elements differ; first at {i} ({where}): "
                             f"got {got[i]!r}, want {expected[i]!r}")


def _mag(rng, n, lo=-3, hi=3):
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(lo, hi, n)).astype(F32)


def _fill_adam(kind, rng, n):
    d = dict(p=_mag(rng, n), g=_mag(rng, n), m=_mag(rng, n), v=np.square(_mag(rng, n)))
    if kind == "zero":
        d.update(g=np.zeros(n, F32), m=np.zeros(n, F32), v=np.zeros(n, F32))
    if kind == "gzero":
        d["g"] = np.where(np.arange(n) % 2 == 0, F32(0.0), F32(-0.0)).astype(F32)
    return d


def _fill_denormal(kind, rng, n):
    """Gradients of 1e-18 .. 1e-20: (1 - beta2) g^2 is denormal or underflows; the moments are of the
    same order (v denormal or near it), and every fourth m and v is zero."""
    g, m = _mag(rng, n, -20, -18), _mag(rng, n, -20, -18)
    v = np.square(_mag(rng, n, -20, -18))
    m[::4], v[::4] = 0, 0
    return dict(p=_mag(rng, n), g=g, m=m, v=v)


def _c_args(a: R.AdamArgs):
    from image_super_resolution_amd import _lib
    return _lib.IsrAdamArgs(*(float(x) for x in a))


def _adam(lib, tb, a, scale=None, guard=None):
    from image_super_resolution_amd import _lib, ops
    ca = _c_args(a)
    _lib.check(lib.isr_mt_adam_guarded(*tb.args(), ctypes.byref(ca), None if scale is None else scale.data_ptr(),
                                       None if guard is None else guard.data_ptr(), ops._stream()), "isr_mt_adam")


def _adam_expected(tb, a, scale=None):
    e = tb.init.copy()
    i = tb.idx
    p, m, v = R.adam_step(e[i["p"]], e[i["g"]], e[i["m"]], e[i["v"]], a, scale)
    e[i["p"]], e[i["m"]], e[i["v"]] = p, m, v
    return e


def _dev_float(x):
    return torch.tensor([x], dtype=torch.float32).to(DEV)


def _guard(a, b):
    return torch.tensor([a, b], dtype=torch.int32).to(DEV)


HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


# ------------------------------------------------------------------ Adam
@pytest.mark.parametrize("t", [1.0, 1000.0])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_bit_for_bit(lib, wd, t):
    """One launch over LAYOUT at the bias corrections of step 1 (bc2_sqrt = 0.0316) and step 1000
    (0.795), data randn scaled over 1e-3 .. 1e3: p, m and v equal optim_ref.adam_step in every bit, and
    nothing else in the arena changed.  Without weight decay the g = m = v = 0 block returns p itself."""
    a = R.adam_args(weight_decay=wd, t=t, **HYPER)
    tb = Tables(LAYOUT, "pgmv", _fill_adam, seed=int(t) + (7 if wd else 0))
    want = _adam_expected(tb, a)
    changed = (want.view(np.int32) != tb.init.view(np.int32)).sum()
    assert changed > 2.5 * tb.idx["p"].size  # the reference moves nearly every p, m and v
    _adam(lib, tb, a)
    tb.check(want, "isr_mt_adam")
    if wd == 0.0:
        zero = [k for k, c in enumerate(tb.chunks) if LAYOUT[c[0]]["kind"] == "zero"]
        assert zero
        for k in zero:
            i = tb.idx["p"][tb.bounds[k]:tb.bounds[k + 1]]
            assert np.array_equal(want[i].view(np.int32), tb.init[i].view(np.int32))


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("scale", [0.25, 0.3, 1.0])
def test_adam_scale(lib, scale, wd):
    """isr_mt_adam's device gradient multiplier, which optim.py never passes: 0.25 (exact products),
    0.3 (every g * s rounds), and 1.0, which must also equal the null-scale launch in every bit."""
    a = R.adam_args(weight_decay=wd, t=3.0, **HYPER)
    tb = Tables(LAYOUT, "pgmv", _fill_adam, seed=11)
    s = _dev_float(scale)
    want = _adam_expected(tb, a, F32(scale))
    if scale != 1.0:
        assert (want != _adam_expected(tb, a)).sum() > tb.idx["p"].size
    _adam(lib, tb, a, scale=s)
    tb.check(want, f"isr_mt_adam, scale {scale}")
    assert s.item() == F32(scale)
    if scale == 1.0:
        null = Tables(LAYOUT, "pgmv", _fill_adam, seed=11)
        _adam(lib, null, a)
        null.check(want, "isr_mt_adam, null scale")


@pytest.mark.parametrize("t", [1.0, 1000.0])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_adam_denormal_gradients(lib, wd, t):
    """Gradients of 1e-18 .. 1e-20 with moments of the same order: g^2, (1 - beta2) g^2 and v are
    denormal or underflow, sqrtf takes its rescaled branch.  fp32 denormals are on in the library's
    code objects, so this is bit for bit too."""
    a = R.adam_args(weight_decay=wd, t=t, **HYPER)
    tb = Tables(SMALL, "pgmv", _fill_denormal, seed=21)
    want = _adam_expected(tb, a)
    if wd == 0.0:
        v = want[tb.idx["v"]]
        assert ((v != 0) & (np.abs(v) < 2.0 ** -126)).sum() > v.size // 4  # denormal results are there
    _adam(lib, tb, a)
    tb.check(want, "isr_mt_adam, denormal gradients")


# ------------------------------------------------------------------ guard
def test_adam_guard(lib):
    """guard[0] == guard[1] (and the null guard of the tests above) updates, to the same bits;
    guard[0] != guard[1] leaves p, m and v, and everything else, untouched.  The give-up is simulated
    by writing the two words, as the chain tests do with state[2]."""
    a = R.adam_args(weight_decay=1e-2, t=2.0, **HYPER)
    for words, updates in [((3, 3), True), ((0, 0), True), ((3, 4), False), ((1, 0), False), ((0, -1), False)]:
        tb = Tables(LAYOUT, "pgmv", _fill_adam, seed=31)
        g = _guard(*words)
        _adam(lib, tb, a, guard=g)
        tb.check(_adam_expected(tb, a) if updates else tb.init, f"isr_mt_adam_guarded, guard {words}")
        assert g.tolist() == list(words)  # the guard words are only read


def _fill_ema_exact(kind, rng, n):
    """Integers in +-2047 times a power of two: x d and y (1 - d) are exact for d = k / 16."""
    def one():
        return (rng.integers(-2047, 2048, n) * 2.0 ** rng.integers(-8, 9, n)).astype(F32)
    return dict(p=one(), g=one())


def _fill_ema_randn(kind, rng, n):
    return dict(p=_mag(rng, n), g=_mag(rng, n))


def _lerp(lib, tb, d, guard=None):
    from image_super_resolution_amd import _lib, ops
    _lib.check(lib.isr_mt_lerp_guarded(*tb.args(), float(d), None if guard is None else guard.data_ptr(),
                                       ops._stream()), "isr_mt_lerp")


def _ema_expected(tb, d):
    e = tb.init.copy()
    e[tb.idx["p"]] = R.ema(e[tb.idx["p"]], e[tb.idx["g"]], d)
    return e


def test_lerp_guard(lib):
    """The same for isr_mt_lerp_guarded and the EMA tensor."""
    for words, updates in [((5, 5), True), ((5, 6), False), ((1, 0), False)]:
        tb = Tables(LAYOUT, "pg", _fill_ema_exact, seed=32)
        _lerp(lib, tb, 0.75, guard=_guard(*words))
        tb.check(_ema_expected(tb, 0.75) if updates else tb.init, f"isr_mt_lerp_guarded, guard {words}")


def test_scale_and_sumsq_take_no_guard(lib):
    """isr_mt_scale and isr_mt_sumsq have no guard argument (the gradient clip of a given-up step is
    harmless: Adam then skips), and isr_mt_scale's launch of the shared kernel is unguarded."""
    from image_super_resolution_amd import _lib
    assert len(_lib.SIGNATURES["isr_mt_scale"][1]) == 5 and len(_lib.SIGNATURES["isr_mt_sumsq"][1]) == 5
    assert len(_lib.SIGNATURES["isr_mt_lerp_guarded"][1]) == len(_lib.SIGNATURES["isr_mt_lerp"][1]) + 1


# ------------------------------------------------------------------ sum of squares
def _fill_int(kind, rng, n):
    return dict(g=rng.integers(-3, 4, n).astype(F32))


def _fill_g(kind, rng, n):
    return dict(g=_mag(rng, n))


def _g_tables(fill, seed):
    """LAYOUT for a kernel that reads g alone: the g slices one float off the grid are the which == 1
    tensors; the others are further aligned ones."""
    return Tables(LAYOUT, "g", fill, seed)


def _sumsq(lib, tb):
    from image_super_resolution_amd import _lib, ops
    buf = torch.full((tb.n + 32,), SENTINEL, device=DEV)
    _lib.check(lib.isr_mt_sumsq(*tb.args(), buf[16:].data_ptr(), ops._stream()), "isr_mt_sumsq")
    torch.cuda.synchronize()
    buf = buf.cpu().numpy()
    assert (buf[:16] == SENTINEL).all() and (buf[16 + tb.n:] == SENTINEL).all(), "a partial outside [0, nchunks)"
    return buf[16:16 + tb.n]


def _chunk_sums64(tb):
    g = tb.init[tb.idx["g"]].astype(np.float64)
    return np.array([np.sum(np.square(g[tb.bounds[k]:tb.bounds[k + 1]])) for k in range(tb.n)])


def test_sumsq_exact_on_integers(lib):
    """g drawn from {-3 .. 3}: a full chunk sums to at most 9 * 65536 < 2^24, so every fp32 partial sum
    is exact whatever the order and partial[k] is the integer sum of chunk k.  g is only read."""
    tb = _g_tables(_fill_int, 41)
    got = _sumsq(lib, tb)
    want = _chunk_sums64(tb)
    assert want.max() < 2 ** 24 and want.max() > 3 * CHUNK
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"chunks {[tb.chunks[k] for k in bad[:5]]}: got {got[bad[:5]]}, want {want[bad[:5]]}"
    tb.check(tb.init, "isr_mt_sumsq")


def test_sumsq_randn_within_gamma_n(lib):
    """|partial - ref64| <= gamma_n * sum g^2, gamma_n = n u / (1 - n u), u = 2^-24, n the fp32
    roundings on the longest path through mt_sumsq_kernel for a chunk of len elements: a thread's
    fmaf chain, 4 * ceil(len / 1024) on the float4 path (ceil(len / 256) <= that on the scalar path),
    then the 6 shuffle adds of the wave reduction and the 4 adds over the wave partials:
    n = 4 * ceil(len / 1024) + 10, 266 for a full chunk."""
    tb = _g_tables(_fill_g, 42)
    got = _sumsq(lib, tb).astype(np.float64)
    ref = _chunk_sums64(tb)
    n = np.array([4 * math.ceil(c[2] / 1024) + 10 for c in tb.chunks], dtype=np.float64)
    assert n.max() == 266
    lim = n * R.U / (1 - n * R.U) * ref
    err = np.abs(got - ref)
    print(f"sumsq randn: worst err/bound {(err / lim).max():.3f}")
    assert (err <= lim).all()
    tb.check(tb.init, "isr_mt_sumsq")


# ------------------------------------------------------------------ clip coefficient
def _clip_coef(lib, partials, max_norm):
    from image_super_resolution_amd import _lib, ops
    n = len(partials)
    buf = torch.full((n + 32,), SENTINEL, device=DEV)
    buf[16:16 + n] = torch.from_numpy(np.asarray(partials, dtype=F32)).to(DEV)
    before = buf.clone()
    out = torch.full((8,), SENTINEL, device=DEV)
    _lib.check(lib.isr_clip_coef(buf[16:].data_ptr(), n, float(max_norm), out[2:].data_ptr(), ops._stream()),
               "isr_clip_coef")
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), "the partials were written"
    out = out.cpu().numpy()
    assert (out[:2] == SENTINEL).all() and (out[4:] == SENTINEL).all()
    return out[2], out[3]


def _check_coef(norm, coef, max_norm):
    """out[1] is optim_ref.clip_coef at the kernel's own out[0]: one fp32 add, one fp32 divide, the clamp."""
    want = R.clip_coef(None, max_norm, norm=norm)[1]
    if np.isnan(want):
        assert np.isnan(coef), f"coefficient {coef!r} for norm {norm!r}: torch.clamp keeps NaN"
    else:
        assert F32(coef).view(np.int32) == want.view(np.int32), f"coefficient {coef!r}, want {want!r} (norm {norm!r})"


CLIP_N = [1, 63, 64, 255, 256, 257, 1000]


@pytest.mark.parametrize("n", CLIP_N)
def test_clip_coef_perfect_squares(lib, n):
    """Partials that sum to 9, 1024 and 10000^2 in n pieces (the last piece large, so a dropped tail
    shows): every piece and every partial sum is an integer below 2^53, the double sum is exact and so
    is its root."""
    for root in (3, 32, 10000):
        total = root * root
        small = min(total // 2 // max(n - 1, 1), 4096)
        parts = [float(small)] * (n - 1) + [float(total - small * (n - 1))]
        assert sum(parts) == total and all(F32(x) == x for x in parts) and parts[-1] >= small
        for max_norm in (10.0, 2.5):
            norm, coef = _clip_coef(lib, parts, max_norm)
            assert norm == root, (root, n, norm)
            _check_coef(norm, coef, max_norm)
            assert coef == 1.0 if root + 1e-6 <= max_norm else coef < 1.0


def test_clip_coef_accumulates_in_double(lib):
    """A perfect square that an fp32 accumulation cannot reach.  8191^2 = 67092481 as 67092472 in the
    last of 1000 partials plus eight pieces of 1.125, one in each group of partials that meets the
    large one's running sum at another add of the kernel's reduction (its own thread's, the partners
    of the six shuffle steps of lane 39 of wave 3, the other waves).  In fp32 each 1.125 is below half
    a last place (2) of the running sum and is lost, the root of 67092472 rounds to 8190.9995, one
    fp32 below; in double every sum is exact."""
    parts = np.zeros(1000, dtype=F32)
    parts[999] = 67092472.0
    assert F32(67092472.0) == 67092472 and 999 % 256 == 231
    for thread in (231, 192 + (39 ^ 32), 192 + (39 ^ 16), 192 + (39 ^ 8), 192 + (39 ^ 4), 192 + (39 ^ 2),
                   192 + (39 ^ 1), 0):
        parts[thread] = 1.125
    assert float(np.sum(parts.astype(np.float64))) == 8191.0 ** 2
    assert F32(math.sqrt(67092472.0)) != 8191
    norm, coef = _clip_coef(lib, parts, 10.0)
    assert norm == 8191.0, repr(norm)
    _check_coef(norm, coef, 10.0)


@pytest.mark.parametrize("n", CLIP_N)
def test_clip_coef_general_sums(lib, n):
    """Partials spread over 1e-6 .. 1e6 with 4e6 in the last: out[0] is fp32(sqrt(float64 sum)) or an
    fp32 neighbour of it (one ulp for the device's double sqrt and the order of the double sum, nothing
    else), out[1] the reference coefficient at out[0]."""
    rng = np.random.default_rng(50 + n)
    parts = (10.0 ** rng.uniform(-6, 6, n)).astype(F32)
    parts[-1] = 4e6
    for max_norm in (10.0, 1e5):
        norm, coef = _clip_coef(lib, parts, max_norm)
        want = R.clip_coef(parts, max_norm)[0]
        assert abs(int(F32(norm).view(np.int32)) - int(want.view(np.int32))) <= 1, (norm, want)
        _check_coef(norm, coef, max_norm)
        assert (coef == 1.0) == (max_norm == 1e5)
    if n > 1:  # the tail matters: without it the norm is another number
        assert R.clip_coef(parts[:-1], 10.0)[0] < 0.999 * want


@pytest.mark.parametrize("n", [1, 257, 1000])
def test_clip_coef_branches(lib, n):
    """Norm below max_norm: exactly 1.0; all-zero partials: norm 0, coefficient 1.0; an inf partial:
    norm inf, coefficient 0; a NaN partial: norm NaN and a NaN coefficient, as torch.clamp(max=1.0)
    gives (a `coef < 1 ? coef : 1` clamp returned 1.0 here and clip_grad_norm_ left NaN gradients be)."""
    rng = np.random.default_rng(60 + n)
    norm, coef = _clip_coef(lib, np.full(n, 0.25 / n, dtype=F32), 10.0)
    assert 0 < norm < 1 and coef.view(np.int32) == F32(1.0).view(np.int32)
    norm, coef = _clip_coef(lib, np.zeros(n, dtype=F32), 10.0)
    assert norm == 0 and not np.signbit(norm) and coef.view(np.int32) == F32(1.0).view(np.int32)
    for where in {0, n // 2, n - 1}:
        parts = (10.0 ** rng.uniform(-3, 3, n)).astype(F32)
        parts[where] = np.inf
        norm, coef = _clip_coef(lib, parts, 10.0)
        assert norm == np.inf and coef == 0 and not np.signbit(coef)
        parts[where] = np.nan
        norm, coef = _clip_coef(lib, parts, 10.0)
        assert np.isnan(norm)
        assert np.isnan(coef), f"NaN norm gave coefficient {coef!r}"
        _check_coef(norm, coef, 10.0)


# ------------------------------------------------------------------ scale
@pytest.mark.parametrize("k", [0.5, 0.3, 0.0, 1.0])
def test_scale_is_one_multiply(lib, k):
    """g *= *coef with the coefficient a device float: torch's own fp32 product of the same device
    values, bit for bit (k = 0 keeps the sign of g in the zero), and nothing else in the arena."""
    from image_super_resolution_amd import _lib, ops
    tb = _g_tables(_fill_g, 71)
    kd = _dev_float(k)
    i = torch.from_numpy(tb.idx["g"]).to(DEV)
    want = tb.arena.clone()
    want[i] = want[i] * kd
    _lib.check(lib.isr_mt_scale(*tb.args(), kd.data_ptr(), ops._stream()), "isr_mt_scale")
    tb.check(want.cpu().numpy(), f"isr_mt_scale, k = {k}")
    assert kd.item() == F32(k)


def _params(shapes, fill):
    ps = []
    for k, s in enumerate(shapes):
        p = torch.zeros(s, device=DEV)
        if len(s) == 4 and k % 2:
            p = p.to(memory_format=torch.channels_last)
        p.requires_grad_()
        p.grad = fill(p)
        ps.append(p)
    return ps


CLIP_SHAPES = [(70001,), (7,), (2 * CHUNK + 5,), (8, 16, 3, 3), (1028,), (0,), (1, 1)]


def test_clip_grad_norm_exact_on_integers():
    """optim.clip_grad_norm_ end to end on gradients from {-3 .. 3}: the partials are exact integers,
    so the returned norm is fp32(sqrt(sum)) within the one ulp of the device's double sqrt, the
    coefficient is the reference's at that norm and every gradient is its one fp32 product with it."""
    from image_super_resolution_amd import optim
    gen = torch.Generator().manual_seed(81)
    ps = _params(CLIP_SHAPES, lambda p: torch.randint(-3, 4, p.shape, generator=gen).float().to(DEV).contiguous(
        memory_format=torch.channels_last if p.dim() == 4 and not p.is_contiguous() else torch.contiguous_format))
    before = [p.grad.cpu().numpy().copy() for p in ps]
    total = sum(int(np.square(g.astype(np.int64)).sum()) for g in before)
    norm = optim.clip_grad_norm_(ps, 10.0)
    torch.cuda.synchronize()
    norm = F32(norm.item())
    want = F32(math.sqrt(total))
    assert abs(int(norm.view(np.int32)) - int(want.view(np.int32))) <= 1, (norm, want)
    coef = R.clip_coef(None, 10.0, norm=norm)[1]
    assert 0 < coef < 0.05
    for p, g0 in zip(ps, before):
        assert np.array_equal(p.grad.cpu().numpy().view(np.int32), (g0 * coef).view(np.int32))


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_clip_grad_norm_nonfinite_is_torchs(bad):
    """One NaN entry: the norm is NaN and every gradient of every tensor becomes NaN, as
    torch.nn.utils.clip_grad_norm_ makes them (clamp keeps the NaN coefficient).  One inf entry: norm
    inf, coefficient 0, finite entries 0 and the inf entry NaN.  error_if_nonfinite raises in both."""
    from image_super_resolution_amd import optim
    shapes = [(70001,), (7,), (8, 16, 3, 3), (1028,)]
    gen = torch.Generator().manual_seed(82)

    def make():
        ps = _params(shapes, lambda p: torch.randn(p.shape, generator=gen).to(DEV))
        ps[0].grad[CHUNK + 3] = bad
        return ps

    gen.manual_seed(82)
    a = make()
    gen.manual_seed(82)
    b = make()
    na = optim.clip_grad_norm_(a, 10.0)
    nb = torch.nn.utils.clip_grad_norm_(b, 10.0)
    assert torch.equal(torch.isnan(na), torch.isnan(nb)) and (math.isnan(bad) or na.item() == nb.item() == math.inf)
    for x, y in zip(a, b):
        assert torch.equal(torch.isnan(x.grad), torch.isnan(y.grad))
        assert torch.equal(x.grad.nan_to_num(nan=5.0), y.grad.nan_to_num(nan=5.0))
    if math.isnan(bad):
        assert all(bool(torch.isnan(x.grad).all()) for x in a)
    else:
        assert int(sum(torch.isnan(x.grad).sum() for x in a)) == 1 and bool(torch.isnan(a[0].grad[CHUNK + 3]))
        assert all(bool((x.grad.nan_to_num(nan=0.0) == 0).all()) for x in a)
    with pytest.raises(RuntimeError, match="non-finite"):
        optim.clip_grad_norm_(make(), 10.0, error_if_nonfinite=True)


# ------------------------------------------------------------------ EMA
@pytest.mark.parametrize("d", [0.5, 0.75, 0.9375])
def test_lerp_exact_products(lib, d):
    """Integers in +-2047 times 2^-8 .. 2^8 and d = k / 16: x d and y (1 - d) are exact in fp32, so
    the result is the single rounding of the exact sum however the compiler contracts x d + y e.
    Over LAYOUT, whose which == 1 tensors have p aligned and g one float off."""
    tb = Tables(LAYOUT, "pg", _fill_ema_exact, seed=91)
    want = _ema_expected(tb, d)
    _lerp(lib, tb, d)
    tb.check(want, f"isr_mt_lerp, d = {d}")


@pytest.mark.parametrize("d", [0.9999 * (1 - math.exp(-1 / 10)), 0.9999])
def test_lerp_general_d_within_derived_bound(lib, d):
    """ModelEMA's first and limiting decay on randn data against the float64 value of
    x d + y (1 - d): |err| <= 2^-21 (|x d| + |y (1 - d)|), test_gpu_glue.py's bar for an fp32
    two-product sum with or without contraction (two products, the sum and the fp32 1 - d: four
    roundings of at most 2^-24 of that magnitude each, doubled).  Everything outside the chunks' p is
    compared bit for bit."""
    tb = Tables(LAYOUT, "pg", _fill_ema_randn, seed=92)
    _lerp(lib, tb, d)
    torch.cuda.synchronize()
    got = tb.arena.cpu().numpy()
    ip, ig = tb.idx["p"], tb.idx["g"]
    df = np.float64(F32(d))
    px, py = tb.init[ip].astype(np.float64) * df, tb.init[ig].astype(np.float64) * (1.0 - df)
    err = np.abs(got[ip].astype(np.float64) - (px + py))
    lim = 2.0 ** -21 * (np.abs(px) + np.abs(py))
    print(f"lerp d={d}: worst err/bound {(err / lim).max():.3f}")
    assert (err <= lim).all()
    assert (got[ip] != tb.init[ip]).mean() > 0.9
    rest = tb.init.copy()
    rest[ip] = got[ip]
    tb.check(rest, "isr_mt_lerp outside p")
