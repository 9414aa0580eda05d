"""The Map step of the header-chain MapReduce from a compiled C++ host (tests/cpp/host_chain_leaves.cpp: g++, the C ABI only): the exported leaf
recording and the raw bytes of four headers go glp_header_chain_leaf_inputs -> glp_witness_eval_device -> glp_witness_place_batch ->
glp_plonk_prove_batch, and the two leaf proofs equal, byte for byte, the ones the Python Map step makes for the same chain (device_witness,
host-built input vectors, one group of two).  The host also hashes the headers through glp_tm_merkle_root_batch and compares.  6 queries,
4 PoW bits."""
import hashlib
import importlib
import os
import random
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chain_inputs_cases as cases  # noqa: E402
from conftest import ROOT, poseidon_consts  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

NQ, PW = 6, 4


@pytest.mark.gpu
def test_cpp_host_proves_the_chain_leaves(pkg, prover, tmp_path):
    dm = importlib.import_module(graft.PKG_NAME + ".data_commitment_mr")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    mr = dm.HeaderChainMapReduce(prover, consts, leaf_headers=2, fan_in=2, num_queries=NQ, pow_bits=PW, device_witness=True, device_witness_chunk=2,
                                 prove_batch=2)
    try:
        mr._record_leaf()
        rng = random.Random(99)
        start, first = hashlib.sha256(b"a trusted header").digest(), 2_500_000
        headers = cases.make_chain(rng, cases.FIELD_LENGTHS, 4, first, start)
        hashes = [start] + [dm.HeaderChainMapReduce.header_hash(h) for h in headers]
        leaves = mr._map_chain(hashes, first, headers, 0, 4)                       # the Python Map step: header_hash, _chain_leaf_inputs on the host
        mr.leaf_program.export_raw(str(tmp_path / "leaf"))
        with open(tmp_path / "chain.bin", "wb") as f:
            f.write(np.array(list(cases.FIELD_LENGTHS) + [2, 4, 4], dtype="<u4").tobytes() + np.array([first], dtype="<u8").tobytes() + start)
            f.write(b"".join(x for h in headers for x in h))
        np.concatenate([np.asarray(a, dtype=np.uint64) for a in consts]).astype("<u8").tofile(str(tmp_path / "pc.bin"))
        exe = tmp_path / "host_chain_leaves"
        libdir = os.path.dirname(pkg.LIB_PATH)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "host_chain_leaves.cpp"), "-o", str(exe), "-L", libdir, "-lglprover", "-pthread",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        r = subprocess.run([str(exe), str(tmp_path / "pc.bin"), str(NQ), str(PW), str(tmp_path / "leaf"), str(tmp_path / "chain.bin"),
                            str(tmp_path / "proof")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout
        assert "input launches 4 syncs 1" in r.stdout and "status 0 0 0 0" in r.stdout and "tree launches 2 syncs 1" in r.stdout, r.stdout
        lines = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines() if " " in ln)
        assert lines["end_hash"] == hashes[-1].hex()
        assert int(lines["key0"]) == int(mr.leaf_circuit.cap()[0])
        for i in range(2):
            proof = (tmp_path / f"proof{i}.bin").read_bytes()
            assert proof == leaves[i], f"leaf {i} is not the Map step's proof"
            assert [int(v) for v in lines[f"public{i}"].split()] == [int(v) for v in pkg.proof_public_inputs(proof)]
    finally:
        mr.free()
