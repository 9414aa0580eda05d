"""GPU parity tests for the radix-32 (32 elements per work-item, log_e = 5) instantiations of glp_ntt_pass_kernel and for the launch logic
around them (XCD tile remap, buffer routing of out-of-place strided calls), word for word against the CPU oracle.

The emulator (tests/emu) proves the index arithmetic of these kernels; only the GPU proves what the gfx950 compiler made of each
instantiation (registers, spills, launch bounds, LDS sizing, the scheduler flags of the radix-32 translation units).  Every case first asserts
through describe_plan that the planner kept the pass structure the case is there for (it clamps tile widths silently).

Which case launches which radix-32 instantiation (tile, mode, direction x form); "fwd+inv" = both directions in the same case:

  tile  mode        form            case
  2^9   STRIP       PLAIN           test_natural_order[15-9:3:5,6:4], [18-9:3:5,9:3:5]                         fwd+inv
  2^10  STRIP       PLAIN, runtime  test_natural_order[16-10:3:5,6:4]                                         fwd+inv
  2^10  STRIP       PLAIN, CT = 4   test_natural_order[16-10:4:5,6:4], [20-10:4:5,10:3:5]                      fwd+inv
  2^11  STRIP       PLAIN           test_natural_order[17-11:3:5,6:3]                                         fwd+inv
  2^12  STRIP       PLAIN           test_natural_order[18-12:2:5,6:4]                                         fwd+inv
  2^9   FINAL_T     PLAIN           test_natural_order[15-6:4,9:3:5], [18-9:3:5,9:3:5]                         fwd+inv
  2^10  FINAL_T     PLAIN           test_natural_order[16-6:4,10:3:5], [20-10:4:5,10:3:5]                      fwd+inv
  2^11  FINAL_T     PLAIN           test_natural_order[17-6:4,11:2:5]                                         fwd+inv
  2^12  FINAL_T     PLAIN           test_natural_order[18-6:4,12:1:5]                                         fwd+inv
  2^9..2^12 STRIP   general         test_bit_reversed[<every strip plan above>] (bit-reversed strips)         fwd+inv
                                    test_coset_lde[15-1-2-9:3:5,6:4], [16-2-3-10:3:5,6:4], [18-1-1-9:3:5,9:3:5] (coset input scale)  fwd
  2^10  FINAL_ROWS  general         test_bit_reversed[16-6:4,10:3:5], test_single_pass[10-10:2:5]             fwd+inv
                                    test_coset_lde[16-1-1-6:4,10:3:5], [10-3-3-10:2:5]                        fwd
  2^9   FINAL_ROWS  general         test_single_pass[9-9:3:5] (both orders), test_coset_lde[18-1-1-9:3:5,9:3:5]  fwd+inv
  2^11  FINAL_ROWS  general         test_single_pass[11-11:2:5] (both orders), test_coset_lde[11-3-2-11:2:5]  fwd+inv
  2^12  FINAL_ROWS  general         test_single_pass[12-12:1:5] (both orders), test_coset_lde[12-2-1-12:1:5]  fwd+inv
  2^9..2^12 FINAL_T general         unreachable: glp_ntt_args_plain() holds for every FINAL_T launch (FINAL_T is never the first pass, so it
                                    carries no coset scale or twiddle table, and a bit-reversed transform ends in FINAL_ROWS)
  2^10  STRIP       general, natural  tests/test_gpu_ntt_optin.py (GLP_FULL_TW makes a natural-order strip non-plain)

The remap and routing cases re-run instantiations of the table above (and the radix-16 / radix-64 ones named in them) under other launch
parameters: test_xcd_remap_both_sides, test_out_of_place_strided."""
import os
import re

import numpy as np
import pytest

from conftest import P, ptr, rand_field
from test_gpu_ntt import oracle_ntt

pytestmark = pytest.mark.gpu

def parse_plan(text):
    """'10:3:5,6:4' -> [(log_r, log_c, elements per work-item)]"""
    out = []
    for part in text.split(","):
        f = [int(v) for v in part.split(":")]
        out.append((f[0], f[1], 1 << (f[2] if len(f) > 2 else 4)))
    return out


def described(prover, log_n, batch, flags=0):
    """describe_plan parsed: [(mode name, log_r, log_c, elements per work-item)]"""
    text = prover.describe_plan(log_n, batch, flags)
    got = [(m, int(r), int(c), int(e) if e else 16) for m, r, c, e in re.findall(r"(\w+)\(R=2\^(\d+),C=2\^(\d+)(?:,E=(\d+))?\)", text)]
    assert len(got) == text.count("(") and got, text
    return got


def assert_plan(prover, log_n, batch, plan, rev):
    """the planner took the override as written: same tile sizes, E = 32 (or 64) exactly on the passes meant to have it and there the C = 2^k the case
    assumes (a 2^6 tile asked for with 8 columns is widened to one wavefront of work-items: the radix-16 passes are pinned by size and E only), the
    last pass in the mode the output order asks for — a case that lands on another kernel fails here instead of passing vacuously"""
    want = parse_plan(plan)
    got = described(prover, log_n, batch, rev)
    assert [(r, e) for _, r, _, e in got] == [(r, e) for r, _, e in want], (plan, got)
    assert [c for _, _, c, e in got if e >= 32] == [c for _, c, e in want if e >= 32], (plan, got)
    last = "finalRows" if (rev or len(want) == 1) else "finalT"
    assert [m for m, _, _, _ in got] == ["strip"] * (len(want) - 1) + [last], (plan, got)
    return got


def make_input(seed, batch, log_n):
    x = rand_field(np.random.default_rng(seed), (batch, 1 << log_n))
    x[0, :] = P - 1
    return x


def run_in_place(prover, x, log_n, flags):
    d = prover.to_device(x)
    try:
        prover.ntt_ex(d, d, log_n, x.shape[0], flags=flags)
        return d.download(x.shape)
    finally:
        d.free()


STRIP_PLANS = [(15, "9:3:5,6:4"), (16, "10:3:5,6:4"), (16, "10:4:5,6:4"), (17, "11:3:5,6:3"), (18, "12:2:5,6:4")]
FINAL_T_PLANS = [(15, "6:4,9:3:5"), (16, "6:4,10:3:5"), (17, "6:4,11:2:5"), (18, "6:4,12:1:5")]


@pytest.mark.parametrize("log_n,plan", STRIP_PLANS + FINAL_T_PLANS + [(18, "9:3:5,9:3:5"), (20, "10:4:5,10:3:5")])
def test_natural_order(prover, oracle, pkg, log_n, plan):
    """the PLAIN strip and FINAL_T instantiations on every tile size, forward and inverse (the inverse FINAL_T applies the 1/n scale), three
    polynomials in place"""
    batch = 3
    x = make_input(3200 + log_n * 13 + len(plan), batch, log_n)
    prover.set_plan(log_n, plan)
    try:
        assert_plan(prover, log_n, batch, plan, 0)
        for inv in (0, 1):
            got = run_in_place(prover, x, log_n, inv * pkg.NTT_INVERSE)
            assert np.array_equal(got, oracle_ntt(oracle, x, inv, 0)), (plan, inv)
    finally:
        prover.set_plan(log_n, None)


@pytest.mark.parametrize("log_n,plan", STRIP_PLANS + [(16, "6:4,10:3:5")])
def test_bit_reversed(prover, oracle, pkg, log_n, plan):
    """bit-reversed output: the general (non-PLAIN) radix-32 strips, and FINAL_ROWS with its 64-bit restaging behind a radix-16 strip"""
    batch = 3
    x = make_input(3300 + log_n * 13 + len(plan), batch, log_n)
    prover.set_plan(log_n, plan)
    try:
        assert_plan(prover, log_n, batch, plan, pkg.NTT_BITREV)
        for inv in (0, 1):
            got = run_in_place(prover, x, log_n, inv * pkg.NTT_INVERSE + pkg.NTT_BITREV)
            assert np.array_equal(got, oracle_ntt(oracle, x, inv, 1)), (plan, inv)
    finally:
        prover.set_plan(log_n, None)


@pytest.mark.parametrize("log_n,plan", [(9, "9:3:5"), (10, "10:2:5"), (11, "11:2:5"), (12, "12:1:5")])
def test_single_pass(prover, oracle, pkg, log_n, plan):
    """one FINAL_ROWS pass on radix-32 work-items, both output orders, forward and inverse"""
    batch = 3
    x = make_input(3400 + log_n, batch, log_n)
    prover.set_plan(log_n, plan)
    try:
        for rev in (0, 1):
            assert_plan(prover, log_n, batch, plan, rev * pkg.NTT_BITREV)
            for inv in (0, 1):
                got = run_in_place(prover, x, log_n, inv * pkg.NTT_INVERSE + rev * pkg.NTT_BITREV)
                assert np.array_equal(got, oracle_ntt(oracle, x, inv, rev)), (plan, inv, rev)
    finally:
        prover.set_plan(log_n, None)


@pytest.mark.parametrize("log_n,rate_bits,batch,plan", [(15, 1, 2, "9:3:5,6:4"), (16, 2, 3, "10:3:5,6:4"), (16, 1, 1, "6:4,10:3:5"),
                                                        (18, 1, 1, "9:3:5,9:3:5"), (11, 3, 2, "11:2:5"), (12, 2, 1, "12:1:5"),
                                                        (10, 3, 3, "10:2:5")])
def test_coset_lde(prover, oracle, pkg, log_n, rate_bits, batch, plan):
    """the commitment's LDE (by cosets, bit-reversed, input scale fused into the first pass) with the size-n transforms on radix-32 plans ==
    the oracle's padded size-N transform, bit-reversed"""
    shift = 0x123456789ABCDEF if (log_n, rate_bits) == (16, 2) else 7
    c = make_input(3500 + 31 * log_n + rate_bits, batch, log_n)
    want = np.zeros((batch, 1 << (log_n + rate_bits)), dtype=np.uint64)
    oracle.orc_lde_coset(ptr(c), ptr(want), log_n, rate_bits, batch, shift)
    oracle.orc_bitrev_rows(ptr(want), log_n + rate_bits, batch)
    prover.set_plan(log_n, plan)
    try:
        assert_plan(prover, log_n, batch << rate_bits, plan, pkg.NTT_BITREV)      # the by-cosets path plans for batch << rate_bits transforms
        assert np.array_equal(prover.lde(c, rate_bits, shift=shift, bitrev=True), want)
    finally:
        prover.set_plan(log_n, None)


def remap_grid(pass_, log_n, batch):
    """(workgroups, group log2 g, remap on) of one described pass: the grid of glp_pass_grid and the condition of glp_exec_ntt —
    tiles narrower than a 128-byte line (C < 16) are regrouped only when the grid is a multiple of 8 << g"""
    mode, log_r, log_c, _ = pass_
    if mode == "strip":
        grid = batch << (log_n - log_r - log_c)
    else:
        rows = batch << (log_n - log_r)
        grid = (rows + (1 << log_c) - 1) >> log_c
    g = 4 - log_c
    return grid, g, grid % (8 << g) == 0


XCD_CASES = [("6:4,10:3:5", 16, 1, "finalT", 1), ("6:4,11:2:5", 17, 1, "finalT", 2), ("10:3:5,6:4", 16, 0, "strip", 1), ("10:2,6:4", 16, 0, "strip", 2)]


@pytest.mark.parametrize("plan,log_n,which,mode,g", XCD_CASES)
def test_xcd_remap_both_sides(prover, oracle, pkg, plan, log_n, which, mode, g):
    """the XCD tile remap of narrow strips / FINAL_T tiles switches on only when the grid is a multiple of 8 << g: two polynomials put each
    plan on the remapped side, three on the plain side — both must give the oracle's words, forward and inverse"""
    prover.set_plan(log_n, plan)
    try:
        for batch, on in ((2, True), (3, False)):
            got_plan = assert_plan(prover, log_n, batch, plan, 0)
            assert got_plan[which][0] == mode
            if mode == "strip":                                  # the strip remap also needs an axis stride of at least a line
                assert log_n - got_plan[which][1] >= 4
            grid, gg, is_on = remap_grid(got_plan[which], log_n, batch)
            assert (gg, is_on) == (g, on), (plan, batch, grid)
            x = make_input(3600 + log_n * 7 + batch + g, batch, log_n)
            for inv in (0, 1):
                got = run_in_place(prover, x, log_n, inv * pkg.NTT_INVERSE)
                assert np.array_equal(got, oracle_ntt(oracle, x, inv, 0)), (plan, batch, inv)
    finally:
        prover.set_plan(log_n, None)


def test_finalt_xcd_switch_off(prover, oracle, pkg):
    """GLP_FINALT_XCD=0 (read on every call) takes the remap of FINAL_T tiles out: a remap-on case gives the same words without it"""
    plan, log_n, batch = "6:4,10:3:5", 16, 2
    prover.set_plan(log_n, plan)
    try:
        got_plan = assert_plan(prover, log_n, batch, plan, 0)
        assert remap_grid(got_plan[1], log_n, batch)[2]
        x = make_input(3700, batch, log_n)
        with_remap = run_in_place(prover, x, log_n, 0)
        os.environ["GLP_FINALT_XCD"] = "0"
        try:
            without = [run_in_place(prover, x, log_n, inv * pkg.NTT_INVERSE) for inv in (0, 1)]
        finally:
            del os.environ["GLP_FINALT_XCD"]
        assert np.array_equal(without[0], with_remap)
        assert np.array_equal(without[0], oracle_ntt(oracle, x, 0, 0))
        assert np.array_equal(without[1], oracle_ntt(oracle, x, 1, 0))
    finally:
        prover.set_plan(log_n, None)


@pytest.mark.parametrize("log_n,plan", [(16, "10:4:5,6:4"), (16, "6:4,10:3:5"), (18, "6:4,6:4,6:4"), (17, "11:2:6,6:3")])
def test_out_of_place_strided(prover, oracle, pkg, log_n, plan):
    """out of place, polynomials embedded in wider rows on both sides: the buffer routing of a radix-32 plan, a three-pass plan (first strip
    source -> scratch, second in scratch) and a radix-64 plan — values equal the oracle, padding columns untouched, source unchanged"""
    batch, n = 3, 1 << log_n
    x = make_input(3800 + log_n * 5 + len(plan), batch, log_n)
    src = np.full((batch, n + 40), 0xDEAD, dtype=np.uint64)
    src[:, :n] = x
    dst = np.full((batch, n + 8), 0xBEEF, dtype=np.uint64)
    prover.set_plan(log_n, plan)
    ds = dd = None
    try:
        assert_plan(prover, log_n, batch, plan, 0)
        ds = prover.to_device(src)
        for inv in (0, 1):
            dd = prover.to_device(dst)
            prover.ntt_ex(ds, dd, log_n, batch, src_stride=n + 40, dst_stride=n + 8, flags=inv * pkg.NTT_INVERSE)
            got = dd.download(dst.shape)
            dd.free()
            dd = None
            assert np.array_equal(got[:, :n], oracle_ntt(oracle, x, inv, 0)), (plan, inv)
            assert np.all(got[:, n:] == 0xBEEF), (plan, inv)
            assert np.array_equal(ds.download(src.shape), src), (plan, inv)
    finally:
        prover.set_plan(log_n, None)
        for d in (ds, dd):
            if d is not None:
                d.free()


def test_radix32_suite_under_the_alternative_two_adic_generator():
    """the radix-32 butterflies use other shift twiddles under the other two-adic generator (w_64 = 2^3 instead of 2^39): this file's whole
    suite once more in a child process against lib/libglprover_altgen.so, the oracle switched to the same generator by conftest"""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    alt = os.path.join(os.path.dirname(here), "0-kno-blobstreamx_amd", "lib", "libglprover_altgen.so")
    assert not os.environ.get("GLP_LIB"), "this test selects the library itself (the child run deselects it)"
    assert os.path.exists(alt), "lib/libglprover_altgen.so is not built (make -C 0-kno-blobstreamx_amd/csrc altgen; __graft_entry__.build() does it)"
    env = dict(os.environ, GLP_LIB=alt)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-p", "no:cacheprovider",
                        "-k", "not alternative_two_adic"], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=os.path.dirname(here))
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0, r.stdout[-3000:]
    assert "passed" in tail and "skipped" not in tail and "failed" not in tail, tail
