"""GPU parity tests for the NTT paths that only an environment switch reaches — GLP_FULL_TW (per-element inter-pass twiddle tables built by
glp_build_full_tw_kernel, (tile position, polynomial) workgroup order), GLP_NTT_SPLIT (two halves of a large batch on two streams) and
GLP_NTT_PLAN (a plan override for every size it sums to) — word for word against the CPU oracle.  The switches are read on every call, so
they are set and cleared around the call in this process."""
import ctypes
import os
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import P, ptr, rand_field
from test_gpu_ntt import oracle_ntt

import bench  # noqa: E402  (repo root is on sys.path through conftest)

pytestmark = pytest.mark.gpu


@contextmanager
def env_set(name, value):
    assert name not in os.environ, f"{name} is already set: these tests choose it themselves"
    os.environ[name] = value
    try:
        yield
    finally:
        del os.environ[name]


def transform(prover, x, log_n, flags):
    d = prover.to_device(x)
    try:
        prover.ntt_ex(d, d, log_n, x.shape[0], flags=flags)
        return d.download(x.shape)
    finally:
        d.free()


@pytest.mark.parametrize("log_n,batch,inv,rev,plan", [
    (13, 9, 0, 0, None), (14, 8, 1, 1, None), (16, 8, 0, 0, "10:3,6:4"),
    (16, 12, 1, 0, "10:2,6:4"),          # grid 192, groups of 4 strips: polynomial-minor order together with the XCD remap
    (16, 9, 0, 0, "10:2,6:4"),           # grid 144: remap off
    (18, 9, 0, 0, "6:4,6:4,6:4"),        # two strips, two tables
    (16, 9, 1, 1, "10:3:5,6:4"),
    (16, 8, 0, 0, "10:4:5,6:4"),         # the general radix-32 strip in natural order (a table makes the pass non-plain)
])
def test_full_twiddle_tables(prover, oracle, pkg, log_n, batch, inv, rev, plan):
    """GLP_FULL_TW=1 on batches of at least 8 (GLP_FULL_TW_MIN_BATCH: the table path and the polynomial-minor workgroup order are live):
    the same call with and without the variable, both equal to the oracle"""
    assert batch >= 8 and log_n <= 22
    x = rand_field(np.random.default_rng(4100 + log_n * 11 + batch), (batch, 1 << log_n))
    x[0, :] = P - 1
    flags = inv * pkg.NTT_INVERSE + rev * pkg.NTT_BITREV
    want = oracle_ntt(oracle, x, inv, rev)
    if plan:
        prover.set_plan(log_n, plan)
    try:
        if plan:
            assert prover.describe_plan(log_n, batch, rev * pkg.NTT_BITREV).count("strip") == plan.count(","), plan
            assert ("E=32" in prover.describe_plan(log_n, batch, rev * pkg.NTT_BITREV)) == (":5" in plan)
        with env_set("GLP_FULL_TW", "1"):
            with_table = transform(prover, x, log_n, flags)
        without = transform(prover, x, log_n, flags)
    finally:
        if plan:
            prover.set_plan(log_n, None)
    assert np.array_equal(with_table, want), "GLP_FULL_TW=1 differs from the oracle"
    assert np.array_equal(without, want), "the default path differs from the oracle"


def test_two_stream_split(prover, oracle, pkg):
    """GLP_NTT_SPLIT=1 needs batch << log_n >= 2^26, two passes and scratch: 65 x 2^20 in place, natural order, is the smallest honest shape
    (halves of 32 and 33 polynomials, the second at scratch offset 32 * n) — forward against the fast oracle, every word, then the inverse
    with the switch still on returns the input"""
    oracle.orc_set_num_threads.argtypes = [ctypes.c_int]
    oracle.orc_set_num_threads(bench.effective_cpus())
    log_n, batch = 20, 65
    x = rand_field(np.random.default_rng(4200), (batch, 1 << log_n))
    x[0, :] = P - 1
    plan = prover.describe_plan(log_n, batch)
    assert plan.count("(") >= 2 and "finalT" in plan, plan            # at least two passes, the last through scratch
    d = prover.to_device(x)
    try:
        with env_set("GLP_NTT_SPLIT", "1"):
            prover.ntt_(d, log_n, batch)
            fwd = d.download(x.shape)
            prover.ntt_(d, log_n, batch, inverse=True)
            back = d.download(x.shape)
    finally:
        d.free()
    assert np.array_equal(back, x), "ifft(fft(x)) != x under GLP_NTT_SPLIT=1"
    ref = x.copy()
    oracle.orc_ntt_fast(ptr(ref), log_n, batch, 0)
    assert np.array_equal(fwd, ref), f"65 x 2^20 ({plan}) on two streams differs from the CPU oracle"


def test_plan_from_the_environment(prover, oracle, pkg):
    """GLP_NTT_PLAN applies to every size it sums to and to no other, and an explicit set_plan takes precedence over it"""
    x = rand_field(np.random.default_rng(4300), (2, 1 << 16))
    x[0, :] = P - 1
    want = oracle_ntt(oracle, x)
    default16, default18 = prover.describe_plan(16, 1), prover.describe_plan(18, 1)
    assert "E=32" not in default16
    with env_set("GLP_NTT_PLAN", "10:3:5,6:4"):
        try:
            assert prover.describe_plan(16, 1) == "strip(R=2^10,C=2^3,E=32)+finalT(R=2^6,C=2^4)"
            assert prover.describe_plan(18, 1) == default18
            assert np.array_equal(transform(prover, x, 16, 0), want)
            prover.set_plan(16, "8:4,8:4")
            assert prover.describe_plan(16, 1) == "strip(R=2^8,C=2^4)+finalT(R=2^8,C=2^4)"
            assert np.array_equal(transform(prover, x, 16, 0), want)
        finally:
            prover.set_plan(16, None)
    assert prover.describe_plan(16, 1) == default16
