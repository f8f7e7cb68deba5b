"""GPU: the grid-stride loops of the four sumcheck round kernels in the regime the production sizes run in -- more than
one pass, a last pass that only some workgroups take, and partials left to sumcheck_reduce_kernel -- against the
oracle's MLSumcheck::prove_as_subprotocol, every round message bit for bit.

ZIP_HIP_SUMCHECK_GRID (a test hook) caps the workgroups of a round-kernel launch, so that 2^14 .. 2^17 entries reach what
2^20 .. 2^24 do uncapped; zip_sumcheck_grid_counts says which regime every launch ran in, so that a cap the library
ignored fails here.  With a cap G of at most one workgroup per CU nothing else limits the grid: a round of `half` points
on a kernel with P points per workgroup runs min(ceil(half / P), G) workgroups, and the counters are plain arithmetic.
The last cases run the uncapped launch path on device-resident tables, at sizes the 8-per-CU cap alone makes multi-pass."""
import functools

import numpy as np
import pytest

import _oracle as orc
from test_gpu_sumcheck_products import BENCH_SHAPE, OVERLAP
from test_gpu_sumcheck_products import FIELDS as PRODUCTS_FIELDS
from test_gpu_sumcheck_products import _assert_state_equal, _coeffs, _masks, _residues, _state_of
from test_gpu_sumcheck_wide import COMBS
from test_gpu_sumcheck_wide import FIELDS as WIDE_FIELDS
from test_gpu_sumcheck_wide import _lds_tail_bound

pytestmark = pytest.mark.gpu

BENCH_MODULUS = 106319353542452952636349991594949358997917625194731877894581586278529202198383
TEST_MODULUS_2 = 57316695564490278656402085503
MOD_NO_SPARE = (1 << 256) - 189
MOD_3LIMB = (1 << 190) - 11 * (1 << 64) - 59
FIELDS = [(BENCH_MODULUS, 4), (TEST_MODULUS_2, 2), (MOD_NO_SPARE, 4), (MOD_3LIMB, 3)]  # those of test_gpu_sumcheck.py

# points per workgroup, and the smallest nv at which round 2 (the first folding round) has 128 workgroups' worth
ONE, QUAD, WIDE, PRODUCTS = "one-thread", "quad", "wide", "products"
POINTS = {ONE: 256, QUAD: 64, WIDE: 32, PRODUCTS: 32}
NV = {ONE: 17, QUAD: 15, WIDE: 14, PRODUCTS: 14}
QUAD_KNOB = {ONE: "0", QUAD: "2"}  # ZIP_HIP_SUMCHECK_QUAD; the other two kernels do not read it

R1CS = ("ccs", 4, 3, (0b011, 0b100), (1, -1))       # (M0 z * M1 z - M2 z) * eq
GENERAL = ("ccs", 4, 4, (0b111, 0b101), (5, -7))    # neither coefficient is 1 or -1
ONE_SHAPES = [("product", 1, 1), ("product", 2, 2), ("product", 3, 3), ("product", 4, 4), R1CS, GENERAL]
QUAD_SHAPES = [("product", 2, 2), ("product", 3, 3), ("product", 4, 3), R1CS, ("product", 1, 2)]
def _wide_ccs(K, degree):
    S, c = COMBS[(K, degree)]
    return "ccs", K, degree, tuple(sum(1 << j for j in Si) for Si in S), tuple(c)


WIDE_SHAPES = [s for K, d in ((5, 3), (6, 4), (7, 3), (8, 4)) for s in (_wide_ccs(K, d), ("product", K, d))]
PRODUCTS_SHAPES = [((1, 2), None), (BENCH_SHAPE, None), ((4,) * 8, None), (OVERLAP, None), ((2,), 4)]  # (shape, degree)


def _id(v):
    if isinstance(v, tuple) and isinstance(v[0], str):  # (form, K, degree, ...)
        return "-".join(map(str, v[:3])) + ("-general" if v is GENERAL else "")
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    return {BENCH_MODULUS: "bench4", TEST_MODULUS_2: "q2", MOD_NO_SPARE: "nospare4", MOD_3LIMB: "q3"}.get(v, str(v))


@pytest.fixture(scope="module")
def mods():
    import torch

    from zinc_amd import cabi, pcs

    if cabi.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu tests must run on the MI355X box")
    # the arithmetic of _expected below: a cap of at most one workgroup per CU is the only cap that binds
    assert torch.cuda.get_device_properties(0).multi_processor_count >= 100
    return cabi, pcs


@pytest.fixture
def grid(monkeypatch):
    """sets ZIP_HIP_SUMCHECK_GRID (None: unset) and, for K <= 4, the kernel through ZIP_HIP_SUMCHECK_QUAD"""
    def set_(G, kernel=None):
        for name, v in (("ZIP_HIP_SUMCHECK_GRID", G), ("ZIP_HIP_SUMCHECK_QUAD", QUAD_KNOB.get(kernel))):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    return set_


def _expected(nv, P, G, rounds=None):
    """(multi_pass, uneven_last_pass, reduce_kernel) of the first `rounds` rounds under a cap G <= CUs"""
    multi = uneven = reduce_ = 0
    for rnd in range(1, (nv if rounds is None else rounds) + 1):
        worth = -(-(1 << (nv - rnd)) // P)
        blocks = min(worth, G)
        multi += worth > blocks
        uneven += worth > blocks and worth % blocks != 0
        reduce_ += blocks > 64
    return multi, uneven, reduce_


def _moved(cabi, before):
    return tuple(a - b for a, b in zip(cabi.sumcheck_grid_counts(), before))


def _assert_regime(moved, kernel, G, rounds=None):
    """what the case is there for, and beyond it the exact counts: the host computes them from the grid it launched"""
    nv, P = NV[kernel], POINTS[kernel]
    multi, uneven, reduce_ = moved
    if G == 100:
        assert multi >= 2 and uneven >= 2 and reduce_ >= 2, moved  # round 1 and the first folding round
    elif G == 3:
        # 3 P points per pass: the rounds of 4 P points and more are multi-pass, nv - log2(P) - 2 of them, each with an
        # uneven last pass (a power of two over 3).  That is nv - 8 and more on the kernels of 64 and 32 points per
        # workgroup; the one-thread kernel (256 points) has nv - 10 such rounds at any nv, 7 of its 17 here.
        if kernel != ONE:
            assert multi >= nv - 8, moved
        assert multi == uneven == nv - P.bit_length() - 1 and reduce_ == 0, moved
    else:  # G == 1: the only workgroup takes every pass and is its own last block
        assert multi == nv - P.bit_length() and uneven == 0 and reduce_ == 0, moved
    assert moved == _expected(nv, P, G, rounds), (moved, kernel, G)


@functools.lru_cache(maxsize=None)
def _from_i64(modulus, fl, nv):
    """2^nv field elements from i64 (small and negative values), as the last table of test_gpu_sumcheck_wide._tables8"""
    f = orc.make_field(modulus, fl)
    return orc.field_elems([orc.field_from_i64(f, int(v)) for v in orc.splitmix64(nv + 7, 1 << nv)], fl)


@functools.lru_cache(maxsize=None)
def _tables(modulus, fl, K, nv, i64_last):
    """K tables of 2^nv canonical residues (Montgomery limbs), drawn as test_gpu_sumcheck_products._residues does; the CCS
    forms of the capped cases take their last table from i64 (above 2^17 entries that walk through Python takes too long:
    every table is drawn).  Shared, never written."""
    rng = np.random.default_rng(nv * 1000 + K * 10 + fl)
    t = _residues(rng, modulus, fl, (K, 1 << nv))
    if i64_last and nv <= 17:
        t[K - 1] = _from_i64(modulus, fl, nv)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _case(modulus, fl, nv, form, K, degree, masks=None, c=None, prime=b""):
    """(tables, masks, coefficients as Montgomery ints, oracle msgs, oracle rand, oracle transcript afterwards) of the
    product of K tables or of the CCS form (sum_t c_t prod_{j in masks_t} v_j) * v_last; shared between the caps"""
    f = orc.make_field(modulus, fl)
    tables = _tables(modulus, fl, K, nv, form == "ccs")
    to = orc.new_transcript()
    if prime:
        orc.absorb(to, prime)
    coeffs = None
    if form == "ccs":
        R = 1 << (64 * fl)
        coeffs = [ci % modulus * R % modulus for ci in c]
        msgs, rand = orc.sumcheck_prove(f, tables, degree, list(masks), coeffs, to)
    else:
        msgs, rand = orc.sumcheck_prove_product(f, tables, degree, to)
    for a in (msgs, rand):
        a.setflags(write=False)
    return tables, masks, coeffs, msgs, rand, to


@functools.lru_cache(maxsize=None)
def _products_case(modulus, fl, nv, shape, degree=None, carry=False, prime=b""):
    """test_gpu_sumcheck_products._case at the sizes of this file: (tables, masks, coeffs, degree, msgs, rand, transcript)"""
    masks, K = _masks(shape)
    rng = np.random.default_rng(nv * 1000 + K * 10 + fl)
    if carry:  # every entry and every coefficient q - 1: the largest products, the accumulator's carries run all the way
        tables = np.tile(orc.field_elems([modulus - 1], fl)[0], (K, 1 << nv, 1))
        coeffs = [modulus - 1] * len(masks)
    else:
        tables = _residues(rng, modulus, fl, (K, 1 << nv))
        coeffs = _coeffs(rng, modulus, fl, len(masks))
    if degree is None:
        degree = max(bin(m).count("1") for m in masks)
    to = orc.new_transcript()
    if prime:
        orc.absorb(to, prime)
    msgs, rand = orc.sumcheck_prove_products(orc.make_field(modulus, fl), tables, degree, masks, coeffs, to)
    for a in (tables, msgs, rand):
        a.setflags(write=False)
    return tables, masks, coeffs, degree, msgs, rand, to


def _handle(cabi, modulus, fl, nv, degree, tables, masks, coeffs, products=False):
    comb = None if masks is None else cabi.make_comb(list(masks), orc.field_elems(coeffs, fl))
    return cabi.Sumcheck(tables, nv, degree, cabi.make_field(modulus, fl), comb=comb, products=products)


def _play(cabi, sc, nv, msgs_o, rand_o):
    """every round through zip_sumcheck_round; -> how the grid counters moved"""
    before = cabi.sumcheck_grid_counts()
    r = None
    for i in range(nv):
        assert np.array_equal(sc.round(r), msgs_o[i]), i
        r = rand_o[i]
    sc.free()
    return _moved(cabi, before)


def _play_shape(cabi, kernel, modulus, fl, shape):
    nv = NV[kernel]
    form, K, degree = shape[:3]
    tables, masks, coeffs, msgs_o, rand_o, _ = _case(modulus, fl, nv, form, K, degree, *shape[3:])
    return _play(cabi, _handle(cabi, modulus, fl, nv, degree, tables, masks, coeffs), nv, msgs_o, rand_o)


# ------------------------------------------------------------------ the capped grid, kernel by kernel
@pytest.mark.parametrize("G", [3, 100])
@pytest.mark.parametrize("modulus,fl", FIELDS, ids=_id)
@pytest.mark.parametrize("shape", ONE_SHAPES, ids=_id)
def test_one_thread_kernel(mods, grid, shape, modulus, fl, G):
    """sumcheck_round_kernel (ZIP_HIP_SUMCHECK_QUAD=0), 256 points per workgroup, 2^17 entries.  Under G = 3 the rounds of
    1024 points and more are multi-pass: 7 of the 17 (nv - 10; the nv - 8 of the kernels with 64 and 32 points per
    workgroup is out of this kernel's reach at any nv)."""
    cabi, _ = mods
    grid(G, ONE)
    _assert_regime(_play_shape(cabi, ONE, modulus, fl, shape), ONE, G)


@pytest.mark.parametrize("G", [3, 100])
@pytest.mark.parametrize("modulus,fl", FIELDS, ids=_id)
@pytest.mark.parametrize("shape", QUAD_SHAPES, ids=_id)
def test_quad_kernel(mods, grid, shape, modulus, fl, G):
    """sumcheck_round_quad_kernel in every round (ZIP_HIP_SUMCHECK_QUAD=2), 64 points per workgroup, 2^15 entries"""
    cabi, _ = mods
    grid(G, QUAD)
    _assert_regime(_play_shape(cabi, QUAD, modulus, fl, shape), QUAD, G)


@pytest.mark.parametrize("G", [3, 100])
@pytest.mark.parametrize("modulus,fl", WIDE_FIELDS, ids=_id)
@pytest.mark.parametrize("shape", WIDE_SHAPES, ids=_id)
def test_wide_kernel(mods, grid, shape, modulus, fl, G):
    """sumcheck_round_wide_kernel (five to eight tables), 32 points per workgroup, 2^14 entries"""
    cabi, _ = mods
    grid(G)
    _assert_regime(_play_shape(cabi, WIDE, modulus, fl, shape), WIDE, G)


@pytest.mark.parametrize("G", [3, 100])
@pytest.mark.parametrize("modulus,fl", PRODUCTS_FIELDS, ids=_id)
@pytest.mark.parametrize("shape,degree", PRODUCTS_SHAPES, ids=_id)
def test_products_kernel(mods, grid, shape, degree, modulus, fl, G):
    """sumcheck_round_products_kernel, 32 points per workgroup, 2^14 entries: in OVERLAP a product re-folds the shared
    table from the round's input in the pass in which, and in the passes after which, its owner writes the folded one"""
    cabi, _ = mods
    grid(G)
    nv = NV[PRODUCTS]
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _products_case(modulus, fl, nv, shape, degree)
    sc = _handle(cabi, modulus, fl, nv, degree, tables, masks, coeffs, products=True)
    _assert_regime(_play(cabi, sc, nv, msgs_o, rand_o), PRODUCTS, G)


# ------------------------------------------------------------------ accumulator depth: one workgroup walks every pass
@pytest.mark.parametrize("modulus,fl", PRODUCTS_FIELDS, ids=_id)
def test_products_kernel_accumulator_depth(mods, grid, modulus, fl):
    """Every entry and every coefficient q - 1 under G = 1: 256 passes of seven products, about 1800 unreduced products of
    (q - 1)^2 in a lane's (2 limbs + 1)-limb accumulator before acc_wide_reduce -- more than a lane collects at 2^24
    uncapped.  The largest case is the modulus without a spare bit."""
    cabi, _ = mods
    grid(1)
    nv = NV[PRODUCTS]
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _products_case(modulus, fl, nv, BENCH_SHAPE, carry=True)
    sc = _handle(cabi, modulus, fl, nv, degree, tables, masks, coeffs, products=True)
    _assert_regime(_play(cabi, sc, nv, msgs_o, rand_o), PRODUCTS, 1)


@functools.lru_cache(maxsize=None)
def _carry_case(modulus, fl, nv, K, degree):
    tables = np.tile(orc.field_elems([modulus - 1], fl)[0], (K, 1 << nv, 1))
    msgs, rand = orc.sumcheck_prove_product(orc.make_field(modulus, fl), tables, degree, orc.new_transcript())
    return tables, msgs, rand


@pytest.mark.parametrize("modulus,fl", FIELDS, ids=_id)
@pytest.mark.parametrize("kernel,K,degree", [(ONE, 2, 2), (QUAD, 4, 3)])
def test_accumulator_depth(mods, grid, kernel, K, degree, modulus, fl):
    """tables all q - 1 under G = 1: 256 (one-thread kernel, 2^17) / 256 (quad kernel, 2^15) products per lane in round 1"""
    cabi, _ = mods
    grid(1, kernel)
    nv = NV[kernel]
    tables, msgs_o, rand_o = _carry_case(modulus, fl, nv, K, degree)
    sc = _handle(cabi, modulus, fl, nv, degree, tables, None, None)
    _assert_regime(_play(cabi, sc, nv, msgs_o, rand_o), kernel, 1)


# ------------------------------------------------------------------ the other entry points under the cap
def _prove_and_check(cabi, sc, K, fl, nv, products, before, msgs_o, rand_o, to_after, kernel):
    """one zip_sumcheck_prove under G = 100 with the default tail: messages, challenges, the sponge afterwards; the launch
    counts move as they do without the cap"""
    state = _state_of(cabi, before)
    rounds0, tails0 = cabi.sumcheck_launch_counts()
    grid0 = cabi.sumcheck_grid_counts()
    msgs, rand = sc.prove(state)
    rounds1, tails1 = cabi.sumcheck_launch_counts()
    n_tail = 0 if products else min(_lds_tail_bound(K, fl), nv)
    assert (rounds1 - rounds0, tails1 - tails0) == (nv - n_tail, 1 if n_tail else 0)
    assert np.array_equal(msgs, msgs_o) and np.array_equal(rand, rand_o)
    _assert_state_equal(state, to_after)
    _assert_regime(_moved(cabi, grid0), kernel, 100, rounds=nv - n_tail)
    with pytest.raises(cabi.ZipError, match="not active"):
        sc.round(rand_o[-1])
    sc.free()


@pytest.mark.parametrize("kernel,modulus,fl,shape", [(ONE, BENCH_MODULUS, 4, ("product", 2, 2)), (QUAD, MOD_3LIMB, 3, R1CS),
                                                     (WIDE, TEST_MODULUS_2, 2, WIDE_SHAPES[0])], ids=_id)
def test_prove_in_one_call_under_the_cap(mods, grid, monkeypatch, kernel, modulus, fl, shape):
    cabi, _ = mods
    grid(100, kernel)
    monkeypatch.delenv("ZIP_HIP_SUMCHECK_TAIL", raising=False)  # the default tail
    nv = NV[kernel]
    form, K, degree = shape[:3]
    prime = bytes(range(71))
    tables, masks, coeffs, msgs_o, rand_o, to_after = _case(modulus, fl, nv, form, K, degree, *shape[3:], prime=prime)
    before = orc.new_transcript()
    orc.absorb(before, prime)
    sc = _handle(cabi, modulus, fl, nv, degree, tables, masks, coeffs)
    _prove_and_check(cabi, sc, K, fl, nv, False, before, msgs_o, rand_o, to_after, kernel)


def test_products_prove_in_one_call_under_the_cap(mods, grid):
    cabi, _ = mods
    grid(100)
    modulus, fl, nv, prime = MOD_NO_SPARE, 4, NV[PRODUCTS], bytes(range(135))
    tables, masks, coeffs, degree, msgs_o, rand_o, to_after = _products_case(modulus, fl, nv, BENCH_SHAPE, prime=prime)
    before = orc.new_transcript()
    orc.absorb(before, prime)
    sc = _handle(cabi, modulus, fl, nv, degree, tables, masks, coeffs, products=True)
    _prove_and_check(cabi, sc, len(tables), fl, nv, True, before, msgs_o, rand_o, to_after, PRODUCTS)


def test_two_products_handles_in_flight_under_the_cap(mods, grid):
    """zip_sumcheck_round_begin / _end, the rounds of two handles interleaved, three workgroups each"""
    cabi, _ = mods
    grid(3)
    L = cabi.lib()
    nv = NV[PRODUCTS]
    ca = _products_case(BENCH_MODULUS, 4, nv, BENCH_SHAPE)
    cb = _products_case(MOD_3LIMB, 3, nv, OVERLAP)
    a = _handle(cabi, BENCH_MODULUS, 4, nv, ca[3], *ca[:3], products=True)
    b = _handle(cabi, MOD_3LIMB, 3, nv, cb[3], *cb[:3], products=True)
    out_a = np.zeros((ca[3] + 1, 4), dtype=np.uint64)
    out_b = np.zeros((cb[3] + 1, 3), dtype=np.uint64)
    before = cabi.sumcheck_grid_counts()
    for i in range(nv):
        ra = None if i == 0 else np.ascontiguousarray(ca[5][i - 1])
        rb = None if i == 0 else np.ascontiguousarray(cb[5][i - 1])
        assert L.zip_sumcheck_round_begin(a._h, None if ra is None else ra.ctypes.data) == 0
        assert L.zip_sumcheck_round_begin(b._h, None if rb is None else rb.ctypes.data) == 0
        assert L.zip_sumcheck_round_end(b._h, out_b.ctypes.data) == 0
        assert L.zip_sumcheck_round_end(a._h, out_a.ctypes.data) == 0
        assert np.array_equal(out_a, ca[4][i]) and np.array_equal(out_b, cb[4][i]), i
    a.free()
    b.free()
    assert _moved(cabi, before) == tuple(2 * x for x in _expected(nv, POINTS[PRODUCTS], 3))


# ------------------------------------------------------------------ the knob itself
def test_a_value_out_of_range_leaves_the_grid_uncapped(mods, grid):
    """not a number, 0, and one above 8 per CU: the counters move as with the variable unset, and the messages are the
    oracle's"""
    import torch

    cabi, _ = mods
    modulus, fl, nv = BENCH_MODULUS, 4, 10
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _products_case(modulus, fl, nv, BENCH_SHAPE)
    moved = {}
    for G in (None, "junk", "0", 8 * torch.cuda.get_device_properties(0).multi_processor_count + 1, 3):
        grid(G)
        sc = _handle(cabi, modulus, fl, nv, degree, tables, masks, coeffs, products=True)
        moved[G] = _play(cabi, sc, nv, msgs_o, rand_o)
    capped = moved.pop(3)
    assert len(set(moved.values())) == 1, moved
    assert moved[None] == (0, 0, 0)  # 2^9 points are 16 workgroups' worth: one pass, the last workgroup folds
    assert capped == _expected(nv, POINTS[PRODUCTS], 3) and capped[0] > 0  # (and the hook is read per round)


# ------------------------------------------------------------------ the production launch path: no hook
def _device_case(cabi, P, nv, degree, tables, masks, coeffs, msgs_o, rand_o, fl, modulus, products=False):
    """device-resident tables, no cap: round 2 alone has more workgroups' worth of points than the grid ever has (8 per
    CU), so round 1 and the first folding round take several passes; the caller's tables are only read"""
    import torch

    assert (1 << (nv - 2)) // P > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    dev = [torch.from_numpy(np.array(tables[k]).view(np.int64)).cuda() for k in range(len(tables))]
    before = [d.clone() for d in dev]
    moved = _play(cabi, _handle(cabi, modulus, fl, nv, degree, dev, masks, coeffs, products=products), nv, msgs_o, rand_o)
    assert moved[0] >= 2 and moved[2] >= 2, moved
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(dev, before))


@pytest.mark.parametrize("modulus,fl", [(TEST_MODULUS_2, 2), (MOD_3LIMB, 3), (BENCH_MODULUS, 4)], ids=_id)
def test_products_2pow19_device_tables_take_several_passes_and_are_only_read(mods, grid, modulus, fl):
    """OVERLAP: four tables, a shared table, a single factor, a repeated mask, a table in no product"""
    cabi, _ = mods
    grid(None)
    nv = 19
    tables, masks, coeffs, degree, msgs_o, rand_o, _ = _products_case(modulus, fl, nv, OVERLAP)
    _device_case(cabi, POINTS[PRODUCTS], nv, degree, tables, masks, coeffs, msgs_o, rand_o, fl, modulus, products=True)


def test_wide_2pow19_device_tables_fold_in_several_passes_and_are_only_read(mods, grid):
    """K = 5, degree 3, the CCS form, three limbs: round 2, the first that folds, has 4096 workgroups' worth"""
    cabi, _ = mods
    grid(None)
    nv, (form, K, degree, m, c) = 19, WIDE_SHAPES[0]
    tables, masks, coeffs, msgs_o, rand_o, _ = _case(MOD_3LIMB, 3, nv, form, K, degree, m, c)
    _device_case(cabi, POINTS[WIDE], nv, degree, tables, masks, coeffs, msgs_o, rand_o, 3, MOD_3LIMB)


@pytest.mark.parametrize("modulus,fl", [(MOD_NO_SPARE, 4), (MOD_3LIMB, 3)], ids=_id)
def test_quad_2pow20_device_tables_fold_in_several_passes_and_are_only_read(mods, grid, modulus, fl):
    """The R1CS-shaped CCS form under the default ZIP_HIP_SUMCHECK_QUAD: round 1 on the one-thread kernel, every folding
    round on the quad kernel, whose round 2 has 4096 workgroups' worth"""
    cabi, _ = mods
    grid(None, None)
    nv, (form, K, degree, m, c) = 20, R1CS
    tables, masks, coeffs, msgs_o, rand_o, _ = _case(modulus, fl, nv, form, K, degree, m, c)
    _device_case(cabi, POINTS[QUAD], nv, degree, tables, masks, coeffs, msgs_o, rand_o, fl, modulus)
