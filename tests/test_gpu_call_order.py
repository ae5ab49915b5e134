"""GPU (-m gpu): what one batch call leaves behind for the next — the host dispatcher of zstd-jni_amd/csrc/zj_kernels.hip carries state from call to call (DESIGN.md
section 2: one split buffer that four layouts are carved from, the promise that a table range is already zero, a wide buffer with two tenants, one block of counters
at fixed offsets, the decode pools, the scratch limit), and every other test pins a single call, mostly on fresh state.  Here small fixed calls ("kinds",
tests/call_order_cases.py: each asserts the route it took, then every frame against the reference) run in orders: one walk in which every ordered pair of kinds
occurs, named orders for the transitions the dispatcher treats specially, and compress / decompress of the same bytes interleaved.

Everything is deterministic (fixed seeds, no retries, no orders drawn at run time) and every input is valid.  There is no CPU twin: no emulation library compiles
the dispatcher, which needs a device for every line it runs."""
import pytest

import call_order_cases as CO

pytestmark = pytest.mark.gpu

EXECUTED = set()           # the ordered pairs the walk's pieces executed in this session ...
RAN = set()                # ... and the pieces that ran


@pytest.fixture(scope="module")
def gpu(zj):
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    zj.batch.init(0)
    return zj


def scratch(gpu):
    return gpu.lib().zjni_scratch_bytes()


# ---- 1. every ordered pair ----
@pytest.mark.parametrize("piece", range(CO.PIECES))
def test_every_ordered_pair_of_kinds(gpu, oracle_ref, piece):
    """one closed walk over the kinds in which each ordered pair (A, B), A = B included, is a step — cut into pieces that each start from released scratch and can be
    replayed alone.  Every call's route and output is checked; a failure names the pair and the two calls before it."""
    run = CO.pieces()[piece]
    done = set()
    CO.play(gpu, oracle_ref, ["release"] + run, done)
    assert done == CO.pairs_of(run)
    EXECUTED.update(done); RAN.add(piece)


def test_the_walk_covers_the_full_product_of_the_kinds():
    """the plan: the pieces' steps are every ordered pair of kinds, once.  The run: with every piece executed in this session the pairs executed ARE that product (a
    dropped kind, a shortened walk or a piece that did not run fails here); with a selection of pieces, theirs."""
    product = {(a, b) for a in CO.NAMES for b in CO.NAMES}
    assert len(CO.NAMES) >= 25 and len(product) == len(CO.NAMES) ** 2
    runs = CO.pieces()
    planned = [p for run in runs for p in zip(run, run[1:])]
    assert len(planned) == len(product) and set(planned) == product
    print({k: CO.SEEN[k] for k in sorted(CO.SEEN)})
    if RAN == set(range(CO.PIECES)):
        assert EXECUTED == product
    else:
        assert EXECUTED == set().union(*[CO.pairs_of(runs[p]) for p in RAN])


# ---- 2. named orders ----
def test_cleared_range_promise_passes_through_the_wave_route(gpu, oracle_ref):
    """a level-3 lane call queues the clear of its tables for the next call; the small wave route in between touches nothing and hands the promise on; the third call's
    range lies inside the cleared one and skips its memset.  No reallocation on the way."""
    CO.play(gpu, oracle_ref, ["release", "run-flags-large"])
    held = scratch(gpu)
    assert held > 0
    CO.play(gpu, oracle_ref, ["wave-hbm", "run-flags-small"])
    assert scratch(gpu) == held
    CO.play(gpu, oracle_ref, ["wave-hbm", "wave-hbm", "run-small", "wave-hbm", "run-flags-large"])       # ... and on: through two wave calls, to a call without flags, back to the full range
    assert scratch(gpu) == held


def test_table_stride_changes_between_calls(gpu, oracle_ref):
    """384 KiB of tables per frame (level 3), then level 1's stride on fewer frames, then 768 KiB per frame (17 / 16): the cleared range fits neither the layout nor, at
    the end, the size"""
    CO.play(gpu, oracle_ref, ["release", "run-flags-large", "lane-l1-small", "run-17-16-small", "run-17-16-large", "lane-l2-large", "run-flags-small"])


def test_regrow_then_reuse(gpu, oracle_ref):
    """the split buffer is freed and allocated again when a call needs more: the promise about the old range is dropped there; the smaller call behind it reuses the
    larger buffer"""
    CO.play(gpu, oracle_ref, ["release", "run-flags-small"])
    small = scratch(gpu)
    CO.play(gpu, oracle_ref, ["run-flags-large"])
    large = scratch(gpu)
    assert large > small > 0
    CO.play(gpu, oracle_ref, ["run-flags-small"])
    assert scratch(gpu) == large


def test_levels_4_to_8_between_level_3_calls(gpu, oracle_ref):
    """the chain parsers lay [chain tables][records][meta] over the lane pipeline's tables and must drop its promise"""
    CO.play(gpu, oracle_ref, ["release", "run-flags-large", "level5", "run-flags-large", "level5", "run-flags-small", "wave-lds", "run-flags-small"])


@pytest.mark.parametrize("kind", ["run-flags-large", "wide", "multi-l3"])
def test_release_in_between(gpu, oracle_ref, kind):
    CO.play(gpu, oracle_ref, ["release", kind, "release", kind])
    assert scratch(gpu) > 0 or kind == "multi-l3"                # (the wave route's tables are per workgroup, not scratch)


def under_limit(gpu, ref, name):
    """a kind's batch while a scratch limit is set: no wave route for small level-3 batches, no need flags, no clear ahead — so the route is the run machine's without
    flags whatever the kind names, and the frames are the same reference frames"""
    k = CO.KINDS[name]
    datas, want = k.datas(gpu), k.want(gpu, ref)
    with CO.switches(k.env):
        outs = gpu.compress_batch(datas, k.level)
        route = gpu.lib().zjni_last_route()
        assert route == CO.ROUTE_RUN, (name, "under a limit took route", route)
        if name == "wide":
            l3 = CO.lists3(gpu)
            assert k.lists(datas, l3), (name, l3)
    CO.same_frames(name + " under a limit", outs, want, datas)


def test_scratch_limit_on_and_off(gpu, oracle_ref):
    L = gpu.lib()
    try:
        CO.play(gpu, oracle_ref, ["release", "run-flags-large", ("limit", 4 << 30)])
        for name in ("run-flags-large", "wide"):
            under_limit(gpu, oracle_ref, name)
        CO.play(gpu, oracle_ref, ["level5"])
        for name in ("wave-hbm", "run-flags-small"):
            under_limit(gpu, oracle_ref, name)
        CO.play(gpu, oracle_ref, [("limit", 0), "run-flags-large", "wide", "run-flags-small", "wave-hbm"])
    finally:
        L.zjni_set_scratch_limit(0)


@pytest.mark.parametrize("third", ["level5", "wide"])
def test_two_streams(gpu, oracle_ref, third):
    """device-resident calls on two torch streams with nothing between them but what the library does itself: the large call's clear is still queued when the small
    call on the other stream starts, and the third call is back on the first stream"""
    import torch
    CO.play(gpu, oracle_ref, ["release"])
    calls = [CO.DeviceCompress(gpu, oracle_ref, CO.KINDS[name]) for name in ("run-flags-large", "run-flags-small", third)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for rep in range(2):
        for c, st in zip(calls, (s1, s2, s1)):
            with torch.cuda.stream(st):
                c.launch()
    torch.cuda.synchronize()
    for c in calls:
        c.check()


def test_wide_buffer_has_two_tenants(gpu, oracle_ref):
    """the wide buffer holds list B of levels 1-3 ([tables][records][meta][queues][flags] per slice) and the lane slots of levels 5-8 at 4 096 frames and more ([a
    table set per lane slot][records][meta]); its existence also decides whether a level 1-3 call asks for its list counts"""
    big = CO.BIG_LANES
    CO.play(gpu, oracle_ref, ["release", "wide"])
    before = scratch(gpu)
    try:
        big.call(gpu, oracle_ref)
    except AssertionError as e:
        raise AssertionError(f"pair (wide -> big-lanes) failed; {e}") from e
    assert scratch(gpu) > before + (8 << 30)                     # the lane slots' table sets
    CO.play(gpu, oracle_ref, ["wide", "run-flags-large", "wide-sliced"])
    CO.play(gpu, oracle_ref, ["release"])


# ---- 3. compress, then decompress of the same bytes, then compress again ----
@pytest.mark.parametrize("ckind,dkind", [("run-flags-small", "dec-split"), ("multi-l3", "dec-multi")])
def test_compress_and_decompress_of_the_same_bytes_interleaved(gpu, oracle_ref, ckind, dkind):
    """the decode pools and the split decoder's buffer are allocated between two compress calls; the second compress gives the frames of the first, and the GPU's own
    frames decode to the input"""
    CO.play(gpu, oracle_ref, ["release"])
    c, d = CO.KINDS[ckind], CO.KINDS[dkind]
    n = min(c.n, d.n)
    assert c.datas(gpu)[:n] == d.datas(gpu, n)
    first = c.call(gpu, oracle_ref)
    held = scratch(gpu)
    d.call(gpu, oracle_ref, frames=first[:n])
    assert scratch(gpu) > held
    again = c.call(gpu, oracle_ref)
    assert again == first
