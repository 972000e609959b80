"""The argument checks and early returns of the pair tests' nine entry points -- sdice_{fisher,chi2}_{pairs,pair_list}{,_dev}
and sdice_pair_list_pack_dev -- straight through the C ABI, so that no engine wrapper hides an argument: n = 2 junctions,
s = 5 samples, a list of 3 pairs (one reversed, one repeated).

Every case changes ONE argument of an otherwise valid call and names the status and the whole message that comes back; the
strings are what the library gave before its entry points shared one argument check (csrc/pairs.h), so they pin that a call
with a single bad argument is answered as it always was.  After every case the same context takes the valid call and gives
the right p-values (the rational sum and the chi2 restatement of tests/pair_fixtures.py, 1e-9) and n_bad = 0.

Two things that look odd and are meant: the all-pairs HOST forms leave the sample limit to their _dev form, whose name the
message carries; a list on s = 1 is "needs at least two samples" in the _dev forms and an index error in the host forms,
which check the list itself first."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pair_fixtures import P_RTOL_TIGHT, exact_two_sided  # noqa: E402
from oracle import oracle_np as O  # noqa: E402
from splicedice_amd.engine import _ptr  # noqa: E402

gpu = pytest.mark.gpu
OK, ERR_ARG = 0, -1
N, S = 2, 5
MAX_PAIRS = 8192 * 8191 // 2
INCL = np.array([[3, 0, 7, 2, 5], [1, 4, 0, 6, 2]], np.int32)          # (no pair table of these has a zero margin)
EXCL = np.array([[9, 4, 1, 8, 3], [2, 0, 5, 7, 11]], np.int64)
LIST = np.array([[0, 1], [4, 2], [0, 1]], np.int32)
ALL_PAIRS = np.array(list(itertools.combinations(range(S), 2)), np.int32)

# the arguments of every entry point after ctx, in C order; `pairs`: a host list [m][2], `tab`: the packed device table
ENTRIES = {
    "sdice_fisher_pairs": "n s incl excl p",
    "sdice_fisher_pairs_dev": "n s incl excl p",
    "sdice_chi2_pairs": "n s incl excl p n_bad",
    "sdice_chi2_pairs_dev": "n s incl excl p n_bad",
    "sdice_fisher_pair_list": "n s incl excl m pairs p",
    "sdice_fisher_pair_list_dev": "n s incl excl m tab p",
    "sdice_chi2_pair_list": "n s incl excl m pairs p n_bad",
    "sdice_chi2_pair_list_dev": "n s incl excl m tab p n_bad",
    "sdice_pair_list_pack_dev": "s m pairs tab",
}
TESTS = [e for e in ENTRIES if e != "sdice_pair_list_pack_dev"]
T_8192 = "more than 8192 samples per junction is not supported"
T_PAIRS = "more than 33550336 pairs in one list is not supported"
T_RANGE = "pair 1 is (2, 5): column indices must lie in [0, 5)"
T_SELF = "pair 1 pairs column 3 with itself"
T_S1 = "pair 0 is (0, 1): column indices must lie in [0, 1)"
T_WALK = ("junction 0: an inclusion count times another sample's exclusion sum is above 2^53 (largest inclusion count 60, "
          "largest exclusion sum 4503599627370496)")
T_EXCL = "junction 1, sample 2: an exclusion sum of 9007199254740993 is above 2^53"
WALK_COUNTS = dict(incl=np.array([[60, 5, 2, 1, 1], [1, 1, 1, 1, 1]], np.int32),
                   excl=np.array([[1 << 49, 1 << 52, 9, 1, 1], [1, 1, 1, 1, 1]], np.int64))
BOTH_COUNTS = dict(incl=INCL, excl=np.array([[9, 4, 1, 8, 3], [2, 0, (1 << 53) + 1, 7, 11]], np.int64))
WIDE = dict(n=1, s=8193, incl=np.zeros((1, 8193), np.int32), excl=np.ones((1, 8193), np.int64))


def _cases():
    """(entry, what, the one changed argument(s), status, message or None)"""
    out = []
    for e, names in ENTRIES.items():
        names = names.split()
        dev, lst, test = e.endswith("_dev"), "pair_list" in e, e in TESTS
        host = test and not dev

        def add(what, change, text, who=e, status=ERR_ARG):
            out.append((e, what, change, status, None if text is None else f"{who}: {text}"))
        add("ctx NULL", dict(ctx=None), "ctx is NULL")
        for k in ("n", "s", "m"):
            if k in names:
                add(f"{k} negative", {k: -1}, "negative size")
        # (the arrays of the host forms: one row of 8193 samples, which the count check reads)
        add("s 8193", WIDE if host else dict(n=1, s=8193) if test else dict(s=8193), T_8192,
            who=e + "_dev" if host and not lst else e)
        if lst:
            add("m above SD_MAX_PAIRS", dict(m=MAX_PAIRS + 1), T_PAIRS)
        for k in ("incl", "excl", "pairs", "tab", "p"):
            if k in names:
                add(f"{k} NULL", {k: None}, "NULL pointer")
        if "n_bad" in names:
            add("n_bad NULL", dict(n_bad=None), "d_n_bad is NULL" if dev else "n_bad is NULL")
        if test:
            add("n 0", dict(n=0), None, status=OK)
        if lst:
            add("m 0", dict(m=0), None, status=OK)
        if test and not lst:
            add("s 1", dict(s=1), None, status=OK)
        elif dev and test:
            add("list, s 1", dict(s=1), "a pair list needs at least two samples")
        else:
            add("list, s 1", dict(s=1), T_S1)
        if "pairs" in names:
            add("list entry out of range", dict(pairs=np.array([[0, 1], [2, 5], [0, 1]], np.int32)), T_RANGE)
            add("list entry i == j", dict(pairs=np.array([[0, 1], [3, 3], [0, 1]], np.int32)), T_SELF)
        if host:
            fisher = "fisher" in e
            add("count above the walk's range", WALK_COUNTS, T_WALK if fisher else None, status=ERR_ARG if fisher else OK)
            add("count above both ranges", BOTH_COUNTS, T_EXCL)
    return out


CASES = _cases()


def _pvalues(pairs, chi2):
    """the reference of the valid call: [N, len(pairs)]"""
    f = (lambda *t: O.chi2_yates_restated(*t)) if chi2 else exact_two_sided
    return np.array([[f(int(INCL[r, i]), int(INCL[r, j]), int(EXCL[r, i]), int(EXCL[r, j])) for i, j in pairs] for r in range(N)])


WANT = {(lst, chi2): _pvalues(LIST if lst else ALL_PAIRS, chi2) for lst in (False, True) for chi2 in (False, True)}


class World:
    """the valid call's arguments on the host and on the device, and one call with some of them replaced"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.d = dict(incl=ctx.to_device(INCL), excl=ctx.to_device(EXCL), tab=ctx.pair_table(S, LIST),
                      p=ctx.empty((N, len(ALL_PAIRS)), np.float64), n_bad=ctx.empty(1, np.int64))
        self.d_pack = ctx.empty(len(LIST), np.uint32)

    def free(self):
        for a in [*self.d.values(), self.d_pack]:
            a.free()

    def call(self, entry, change):
        """-> (status, message, p as the call left it [N, 10] or None, n_bad as the call left it or None)"""
        names = ENTRIES[entry].split()
        dev = entry.endswith("_dev") and entry in TESTS
        self.p = np.full((N, len(ALL_PAIRS)), -7.25)
        self.bad = C.c_int64(-5)
        self.d["p"].memset(0xAA)
        self.d["n_bad"].memset(0xFF)
        self.d_pack.memset(0xAA)
        if dev:
            args = dict(n=N, s=S, m=len(LIST), **{k: v.ptr for k, v in self.d.items()})
        else:
            args = dict(n=N, s=S, m=len(LIST), incl=INCL, excl=EXCL, pairs=LIST, p=self.p, n_bad=C.byref(self.bad),
                        tab=self.d_pack.ptr)
        args["ctx"] = self.ctx.h
        args.update(change)
        keep = [args[k] for k in names]                                   # (the arrays of this call stay alive)
        argv = [_ptr(a) if isinstance(a, np.ndarray) else a for a in [args["ctx"], *keep]]
        status = getattr(self.ctx.lib, entry)(*argv)
        msg = self.ctx.lib.sdice_last_error().decode()
        self.ctx.sync()
        if entry not in TESTS:
            return status, msg, None, None
        p = self.d["p"].to_host() if dev else self.p
        bad = (int(self.d["n_bad"].to_host()[0]) if dev else self.bad.value) if "n_bad" in names else None
        return status, msg, p, bad

    def valid(self, entry):
        status, msg, p, bad = self.call(entry, {})
        assert status == OK, (entry, msg)
        if entry not in TESTS:
            want = (LIST[:, 0].astype(np.uint32) << 16) | LIST[:, 1].astype(np.uint32)
            assert np.array_equal(self.d_pack.to_host(), want), entry
            return
        lst, chi2 = "pair_list" in entry, "chi2" in entry
        m = len(LIST) if lst else len(ALL_PAIRS)
        np.testing.assert_allclose(p.reshape(-1)[:N * m].reshape(N, m), WANT[lst, chi2], rtol=P_RTOL_TIGHT, atol=0, err_msg=entry)
        assert bad == (0 if chi2 else None), entry


@pytest.fixture(scope="module")
def world(ctx):
    w = World(ctx)
    yield w
    w.free()


@gpu
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_the_valid_call(world, entry):
    world.valid(entry)


@gpu
@pytest.mark.parametrize("entry,what,change,status,message", CASES, ids=[f"{c[0][6:]}-{c[1]}" for c in CASES])
def test_one_changed_argument(world, entry, what, change, status, message):
    got, msg, p, bad = world.call(entry, change)
    assert got == status, (entry, what, got, msg)
    if message is not None:
        assert msg == message
    elif entry in TESTS and what != "count above the walk's range":
        # nothing to do: the output keeps its fill (host -7.25, device 0xAA bytes) and chi2's count is reset
        dev = entry.endswith("_dev")
        assert (p.view(np.uint64) == np.uint64(0xAAAAAAAAAAAAAAAA)).all() if dev else (p == -7.25).all(), (entry, what)
        assert bad == (0 if "chi2" in entry else None), (entry, what, bad)
    world.valid(entry)
