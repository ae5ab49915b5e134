"""The calls ("kinds") and the orders of tests/test_gpu_call_order.py.  TEST INFRASTRUCTURE.

A kind is one small, fixed batch call: its inputs, the product switches it is made under, the route it must take and the reference's answer for every frame.  A
kind's call() makes the call on the GPU, asserts the route FIRST (so a kind can never silently test something else), then every frame.  The frames of all kinds
are cut from one pool (frame k of every batch begins with the same bytes): what a call leaves in tables, records, queues or flags of slot k is then plausible
data for the next call's slot k, and a stale entry that is taken for a fresh one gives a valid but different frame instead of going unnoticed.

Every batch mixes sizes 0, 1, 63, 64 and 65, a few KiB, a run of one byte, noise and text-like synth_host frames."""
import contextlib
import ctypes as C
import os
import random

ROUTE_FUSED, ROUTE_WAVE, ROUTE_LANE, ROUTE_RUN, ROUTE_RUN_FLAGS, ROUTE_OTHER, ROUTE_WAVE_HBM, ROUTE_PIPE = 1, 2, 3, 5, 6, 8, 9, 11      # include/zjni_amd.h ZJNI_ROUTE_*
SWITCHES = ("ZJNI_SPLIT_MIN", "ZJNI_DSPLIT_MIN", "ZJNI_L3_WAVE_MAX", "ZJNI_NEED", "ZJNI_DEC_MB", "ZJNI_WIDE_SLICE")          # product switches, live under the suite's ZJNI_DEBUG_LIVE_SWITCHES
KiB = 1 << 10
BLOCK = 128 * KiB
LDS = dict(hash_log=14, chain_log=13)


@contextlib.contextmanager
def switches(env):
    """exactly `env` of the product switches for the duration of one call, the others unset; what was set before comes back afterwards"""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            if k in env: os.environ[k] = env[k]
            else: os.environ.pop(k, None)
        yield
    finally:
        for k, v in saved.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


# ---- the pool: frame k of every batch is a prefix of pool entry k ----
EDGE = (0, 1, 63, 64, 65, 3000, 5000)
POOL = 208
_pool = {}


def pool(zj):
    """[bytes] x POOL, each 300 000 bytes: entry 7 is a run of one byte, 8 is noise, 9 is a short period, the others the text-like generator's"""
    if "pool" not in _pool:
        text = zj.synth_host(BLOCK, 4000, POOL)
        rnd = random.Random(2323)
        out = []
        for k in range(POOL):
            if k == 7: d = bytes([7]) * 300000
            elif k == 8: d = rnd.randbytes(300000)
            elif k == 9: d = (rnd.randbytes(37) * 8200)[:300000]
            else: d = text[k * BLOCK:(k + 1) * BLOCK] + text[((k + 5) % POOL) * BLOCK:((k + 5) % POOL + 1) * BLOCK] + text[((k + 11) % POOL) * BLOCK:((k + 11) % POOL) * BLOCK + 300000 - 2 * BLOCK]
            assert len(d) == 300000
            out.append(d)
        _pool["pool"] = out
    return _pool["pool"]


def batch(zj, n, sizes):
    """n frames: the edge sizes first, then `sizes` in turn"""
    assert n <= POOL
    p = pool(zj)
    return [p[k][:EDGE[k] if k < len(EDGE) else sizes[(k - len(EDGE)) % len(sizes)]] for k in range(n)]


SMALL, LARGE = 70, 200                                 # two sizes of the lane pipeline's kinds: a following call's tables end inside and beyond the preceding call's
TO_24K = (24000, 16384, 9000, 4096, 700, 20000, 300, 12345)
TO_64K = (65536, 16384, 9000, 40000, 700, 24000, 4096, 65535)
WIDE = (65537, 131072, 9000, 100000, 65536, 70000, 700, 131071)
MULTI = (BLOCK + 1, 300000, BLOCK + 1, 262144)
AROUND_16K = (16384, 16385, 9000, 40000, 700, 20000, 4096, 12000)


SEEN = {}               # kind -> what the library last said about its route and lists (printed by the walk's coverage test)


def lists3(zj):
    a = (C.c_uint * 3)()
    assert zj.lib().zjni_last_lists(a) == 0
    return list(a)


def dlists(zj):
    a = (C.c_uint * 5)()
    assert zj.lib().zjni_last_decode_lists2(a) == 0
    return list(a)              # [0] single-block pipeline, [1] fused kernel, [2] block stages, [3] their blocks, [4] frames of one stored block copied by stage 1


def same_frames(name, got, want, datas):
    for k, (z, w) in enumerate(zip(got, want)):
        assert not isinstance(z, Exception), (name, k, len(datas[k]), z)
        assert z == w, (name, "frame", k, "of", len(datas[k]), "bytes differs from the reference's", len(z), len(w))
    assert len(got) == len(want)


class Compress:
    """zjni_compress_batch2 / _advanced from host pointers.  route: zjni_last_route() behind the call; lists(datas, [A, B, C]) -> bool: what zjni_last_lists must say (it
    synchronises, and only then is ZJNI_ROUTE_PIPE known: route_after)"""

    def __init__(self, name, level, n, sizes, env, route, lists, hash_log=0, chain_log=0, route_after=None):
        self.name, self.level, self.n, self.sizes, self.env, self.route, self.lists = name, level, n, sizes, env, route, lists
        self.hash_log, self.chain_log, self.route_after = hash_log, chain_log, route if route_after is None else route_after
        self._want = None

    def datas(self, zj):
        return batch(zj, self.n, self.sizes)

    def want(self, zj, ref):
        if self._want is None:
            self._want = [ref.compress(d, self.level, False, self.hash_log, self.chain_log) for d in self.datas(zj)]
        return self._want

    def check_route(self, zj, datas):
        L = zj.lib()
        route = L.zjni_last_route()
        assert route == self.route, (self.name, "took route", route, "not", self.route)
        l3 = lists3(zj)
        SEEN[self.name] = (route, tuple(l3))
        assert sum(l3) == len(datas) and self.lists(datas, l3), (self.name, "lists", l3)
        assert L.zjni_last_route() == self.route_after, (self.name, "route behind zjni_last_lists", L.zjni_last_route(), "not", self.route_after)

    def call(self, zj, ref):
        datas, want = self.datas(zj), self.want(zj, ref)
        with switches(self.env):
            outs = zj.compress_batch(datas, self.level, hash_log=self.hash_log, chain_log=self.chain_log)
            self.check_route(zj, datas)
        same_frames(self.name, outs, want, datas)
        return outs


class DeviceCompress:
    """the same call of a Compress kind through zjni_compress_batch_device* on the CURRENT torch stream: prepared ahead (inputs and destinations on the device), launched
    without a wait, read back later"""

    def __init__(self, zj, ref, kind):
        import torch
        self.zj, self.kind = zj, kind
        self.datas, self.want = kind.datas(zj), kind.want(zj, ref)
        self.bounds = [zj.Zstd.compressBound(len(d)) for d in self.datas]
        off = lambda v: torch.tensor([sum(v[:i]) for i in range(len(v) + 1)], dtype=torch.int64, device="cuda")          # noqa: E731
        self.src = torch.frombuffer(bytearray(b"".join(self.datas) or b"\0"), dtype=torch.uint8).cuda()
        self.soff, self.doff = off([len(d) for d in self.datas]), off(self.bounds)
        self.dst = torch.full((sum(self.bounds),), 0x5C, dtype=torch.uint8, device="cuda")
        self.res = torch.full((len(self.datas),), -1, dtype=torch.int64, device="cuda")

    def launch(self):
        k = self.kind
        with switches(k.env):
            self.zj.batch.compress(self.src, self.soff, self.dst, self.doff, k.level, results=self.res, hash_log=k.hash_log, chain_log=k.chain_log)
            route = self.zj.lib().zjni_last_route()              # (host state: no wait)
        assert route == k.route, (k.name, "took route", route, "not", k.route)

    def check(self):
        """(after a synchronise)"""
        host, sizes = self.dst.cpu().numpy().tobytes(), self.res.cpu().tolist()
        at, outs = 0, []
        for b, s in zip(self.bounds, sizes):
            assert 0 < s <= b, (self.kind.name, s, b)
            outs.append(host[at:at + s]); at += b
        same_frames(self.kind.name, outs, self.want, self.datas)


_dict = {}


def dictionary(zj, ref):
    """one raw-content dictionary of JSON-like records and its four digests: (bytes, ZstdDictCompress level 3, ZstdDictDecompress, the reference's CDict)"""
    if "d" not in _dict:
        from util import json_records
        raw = b",".join(json_records(400, seed=3))[:16384]
        _dict["d"] = (raw, zj.ZstdDictCompress(raw, 3), zj.ZstdDictDecompress(raw), ref.CDict(raw, 3))
    return _dict["d"]


def dict_sources(zj, n):
    """records that share the dictionary's vocabulary, the pool's text and noise in between, the edge sizes first; all within the attach range (8 KiB)"""
    from util import json_records
    recs, p = json_records(3000, seed=5, first=100), pool(zj)
    out = []
    for k in range(n):
        size = EDGE[k] if k < len(EDGE) else (8192, 1000, 4096, 130, 2500, 400)[k % 6]
        out.append(p[k][:size] if (k < len(EDGE) or k % 5 == 0 or k in (7, 8, 9)) else b",".join(recs[k * 11:k * 11 + 150])[:size])
    return out


class CompressDict:
    """zjni_compress_batch_usingCDict: the dictionary pipeline keeps its own scratch (cdBuf) and reports no route — it must leave zjni_last_route() as it found it"""
    name, n = "cdict", SMALL

    def call(self, zj, ref):
        raw, cd, dd, ref_cd = dictionary(zj, ref)
        srcs = dict_sources(zj, self.n)
        if not hasattr(self, "_want"):
            self._want = [ref_cd.compress(s) for s in srcs]
        before = zj.lib().zjni_last_route()
        with switches({}):
            outs = zj.compress_batch(srcs, dictionary=cd)
        assert zj.lib().zjni_last_route() == before, (self.name, "changed the route diagnostics", before, zj.lib().zjni_last_route())
        same_frames(self.name, outs, self._want, srcs)


class Decompress:
    """zjni_decompress_batch[_usingDDict] of the reference's frames; lists(datas, zjni_last_decode_lists2) -> bool names the stages the frames must have taken (every
    frame is on a list: all_listed; one the block stages hand over to the fused kernel is on two)"""

    def __init__(self, name, n, sizes, env, lists, level=3, with_dict=False):
        self.name, self.n, self.sizes, self.env, self.lists, self.level, self.with_dict = name, n, sizes, env, lists, level, with_dict
        self._frames = None

    def datas(self, zj, n=None):
        return dict_sources(zj, n or self.n) if self.with_dict else batch(zj, n or self.n, self.sizes)

    def frames(self, zj, ref):
        if self._frames is None:
            if self.with_dict:
                ref_cd = dictionary(zj, ref)[3]
                self._frames = [ref_cd.compress(d) for d in self.datas(zj)]
            else:
                self._frames = [ref.compress(d, (self.level, 1)[k % 5 == 4]) for k, d in enumerate(self.datas(zj))]          # (every fifth frame at level 1: other table logs, other modes)
        return self._frames

    def call(self, zj, ref, frames=None):
        """frames: the first len(frames) inputs from these frames instead of the reference's (the GPU's own, which are the same bytes)"""
        datas = self.datas(zj, None if frames is None else len(frames))
        frames = self.frames(zj, ref) if frames is None else frames
        with switches(self.env):
            outs = zj.decompress_batch(frames, [len(d) for d in datas], dictionary(zj, ref)[2] if self.with_dict else None)
            l = dlists(zj)
        SEEN[self.name] = tuple(l)
        assert self.lists(datas, l), (self.name, "decode lists", l)
        for k, (o, d) in enumerate(zip(outs, datas)):
            assert not isinstance(o, Exception), (self.name, k, len(d), o)
            assert o == d, (self.name, "frame", k, "of", len(d), "bytes does not decode to its input")
        return outs


class Sequences:
    """zjni_compress_sequences_batch_device on a few cases of tests/sequences_cases.py (level 3, no flags: one call), the reference's ZSTD_compressSequences frame each"""
    name = "sequences"

    def call(self, zj, ref):
        import sequences_cases as SC
        from test_gpu_sequences import run_batch
        cases = [c for c in SC.smallest() + SC.from_generator() + SC.multi_block() if c.level == 3 and c.flags == 0]
        assert len(cases) >= 12
        with switches({}):
            got = run_batch(zj, cases)
        for c, g in zip(cases, got):
            SC.check(c, g, ref)


class Generate:
    """zjni_generate_sequences_batch_device on the level-3 frames of generate_cases.small_random: the reference's ZSTD_generateSequences rows, all on the wave route"""
    name = "generate"

    def call(self, zj, ref):
        import generate_cases as GC
        from test_gpu_generate import run_batch, as_list
        cases = [c for c in GC.small_random()[:64] if c.level == 3]
        assert len(cases) == 16
        with switches({}):
            got, last = run_batch(zj, [c.data for c in cases], 3)
        assert last["wave"] == len(cases) and last["lane"] == 0, (self.name, last)
        for c, g in zip(cases, got):
            GC.check(c, as_list(g))


def all_listed(d, l):
    return l[0] + l[2] + l[4] <= len(d) <= l[0] + l[1] + l[2] + l[4]


def _count(datas, lo, hi):
    return sum(1 for d in datas if lo < len(d) <= hi)


def _lane(level, tag, wide):
    """levels 1, 2 and -3 on the lane machine.  wide: at levels 1 and -3 the frames whose tables do not fit the small LDS pass go to the wide launch (list B: these kinds are
    tenants of the wide buffer too); level 2 keeps every frame up to 64 KiB on the common launch"""
    lists = (lambda d, l: l[0] > 0 and l[1] > 0 and l[2] == 0) if wide else (lambda d, l: l == [len(d), 0, 0])
    return [Compress(f"lane-l{tag}-{w}", level, n, TO_24K, {"ZJNI_SPLIT_MIN": "1"}, ROUTE_LANE, lists) for w, n in (("small", SMALL), ("large", LARGE))]


def _run(tag, env, route, **logs):
    only_a = lambda d, l: l == [len(d), 0, 0]              # noqa: E731
    return [Compress(f"{tag}-{w}", 3, n, TO_64K, dict(env, ZJNI_SPLIT_MIN="1"), route, only_a, **logs) for w, n in (("small", SMALL), ("large", LARGE))]


def _kinds():
    """the numbers are those of the list the suite was asked to cover (kinds 4 to 8 in two sizes)"""
    split = {"ZJNI_SPLIT_MIN": "1"}
    wide_lists = lambda d, l: l == [_count(d, -1, 65536), _count(d, 65536, BLOCK), 0]             # noqa: E731
    ks = [
        # 1: the fused kernel; 2: the wave matcher with its tables in LDS; 3: a wave per frame over HBM tables
        Compress("fused-l1", 1, SMALL, TO_64K, {}, ROUTE_FUSED, lambda d, l: l[0] > 0 and l[2] == 0),
        Compress("wave-lds", 3, SMALL, TO_64K, {}, ROUTE_WAVE, lambda d, l: l == [len(d), 0, 0], **LDS),
        Compress("wave-hbm", 3, SMALL, TO_64K, {}, ROUTE_WAVE_HBM, lambda d, l: l == [0, 0, len(d)]),
        # 4, 5: the lane machine at levels 1 and 2 (another table stride)
        *_lane(1, "1", True),
        *_lane(2, "2", False),
        # 6, 7: the run machine with flags for every frame and without; 8: larger tables, another stride (no flags: their bitmaps end at 16 / 15)
        *_run("run-flags", {"ZJNI_NEED": "1"}, ROUTE_RUN_FLAGS),
        *_run("run", {"ZJNI_NEED": "0"}, ROUTE_RUN),
        *_run("run-17-16", {}, ROUTE_RUN, hash_log=17, chain_log=16),
        # 9: frames of 64 KiB + 1 .. 128 KiB on the wide launch, in one slice (with flags) and in two
        Compress("wide", 3, SMALL, WIDE, split, ROUTE_RUN_FLAGS, wide_lists),
        Compress("wide-sliced", 3, SMALL, WIDE, dict(split, ZJNI_WIDE_SLICE="64"), ROUTE_RUN_FLAGS, wide_lists),
        # 10: multi-block frames (list C); at level 3 the whole small batch is list C's and the library names the pipelined pair of waves once the lists are read;
        # at level 1 the route names list A's kernel, list C goes to the same pair
        Compress("multi-l3", 3, 24, MULTI, {}, ROUTE_WAVE_HBM, lambda d, l: l == [0, 0, len(d)], route_after=ROUTE_PIPE),
        Compress("multi-l1", 1, 24, MULTI, {}, ROUTE_FUSED, lambda d, l: l[2] == _count(d, BLOCK, 1 << 30) and l[0] > 0),
        # 11: level 5 on both sides of 16 KiB (list A's chain kernel, list C); 12: level -3 on the lane machine; 13: a dictionary
        Compress("level5", 5, 40, AROUND_16K, {}, ROUTE_OTHER, lambda d, l: l == [_count(d, -1, 16384), 0, _count(d, 16384, BLOCK)]),
        *_lane(-3, "neg3", True),
        CompressDict(),
        # 14: decompress on the fused kernel; 15: the three-stage pipeline (stored frames are copied by stage 1)
        Decompress("dec-fused", SMALL, TO_64K, {}, lambda d, l: all_listed(d, l) and l[0] == 0 and l[2] == 0),
        Decompress("dec-split", 100, TO_64K, {"ZJNI_DSPLIT_MIN": "1"}, lambda d, l: all_listed(d, l) and l[0] >= len(d) // 2 and l[4] > 0),
        # 16: multi-block frames on the block stages — and with the stages switched off: the fused kernel alone, which keeps no lists (the pipeline's counts then
        # still say what the last pipeline call left, so only the stages' own are asserted)
        Decompress("dec-multi", 24, MULTI, {}, lambda d, l: all_listed(d, l) and l[0] == 0 and l[2] == _count(d, BLOCK, 1 << 30) and l[3] >= 2 * l[2]),
        Decompress("dec-multi-off", 24, MULTI, {"ZJNI_DEC_MB": "0"}, lambda d, l: l[2] == 0 and l[3] == 0),
        # 17: a dictionary, through the pipeline (no block stages with a dictionary)
        Decompress("dec-dict", 100, None, {"ZJNI_DSPLIT_MIN": "1"}, lambda d, l: all_listed(d, l) and l[0] > 0 and l[2] == 0, with_dict=True),
        # 18
        Sequences(), Generate(),
    ]
    return {k.name: k for k in ks}


KINDS = _kinds()
NAMES = tuple(KINDS)


def play(zj, ref, steps, executed=None):
    """the steps in order: a kind's name is its call; "release" frees the library's scratch (zjni_release_scratch), ("limit", bytes) sets the scratch limit.  A
    failure names the pair (the step before -> the call that failed) and the two steps before the pair.  executed: gets the pairs of kinds called back to back."""
    L = zj.lib()
    done = []
    for step in steps:
        if step == "release":
            assert L.zjni_release_scratch() == 0 and L.zjni_scratch_bytes() == 0
        elif isinstance(step, tuple):
            assert step[0] == "limit" and L.zjni_set_scratch_limit(step[1]) == step[1]
        else:
            try:
                KINDS[step].call(zj, ref)
            except AssertionError as e:
                raise AssertionError(f"pair ({done[-1] if done else 'nothing'} -> {step}) failed; the two steps before it: {done[-3:-1]}; {e}") from e
            if done and done[-1] in KINDS and executed is not None:
                executed.add((done[-1], step))
        done.append(step)


# ---- orders ----
def euler_walk(names, seed=20231):
    """a closed walk over the complete directed graph on `names`, loops included: every ordered pair (A, B), A = B too, is one step of it exactly once (Hierholzer's
    algorithm; the out-edges of every node shuffled from a fixed seed)"""
    rnd = random.Random(seed)
    out = {a: list(names) for a in names}
    for a in names:
        rnd.shuffle(out[a])
    stack, walk = [names[0]], []
    while stack:
        v = stack[-1]
        if out[v]: stack.append(out[v].pop())
        else: walk.append(stack.pop())
    walk.reverse()
    assert len(walk) == len(names) ** 2 + 1
    return walk


PIECES = 24


def pieces():
    """the walk cut into PIECES runs that overlap by one call: piece p replays its first call on released scratch, so the pair across a cut is the next piece's first"""
    walk = euler_walk(NAMES)
    steps = len(walk) - 1
    cuts = [steps * p // PIECES for p in range(PIECES + 1)]
    return [walk[cuts[p]:cuts[p + 1] + 1] for p in range(PIECES)]


def pairs_of(run):
    return set(zip(run, run[1:]))


class BigLanes(Compress):
    """level 5, 4 096 frames just above 16 KiB: list C on the lane-slot route (zj_enc_match_big_kernel), whose table sets and records live in the WIDE buffer — the
    buffer list B of levels 1-3 uses with another layout.  64 distinct frames, each 64 times (the reference compresses 64); not part of the walk: its scratch is
    ~27 GiB"""

    def __init__(self):
        Compress.__init__(self, "big-lanes", 5, 4096, None, {}, ROUTE_OTHER, lambda d, l: l == [0, 0, len(d)])

    def datas(self, zj):
        p = pool(zj)
        return [p[10 + k % 64][:17 * KiB + k % 64] for k in range(self.n)]

    def want(self, zj, ref):
        if self._want is None:
            d = self.datas(zj)
            first = [ref.compress(x, 5) for x in d[:64]]
            self._want = [first[k % 64] for k in range(self.n)]
        return self._want


BIG_LANES = BigLanes()
