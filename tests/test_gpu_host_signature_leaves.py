"""The Map step of the signature MapReduce from a compiled C++ host (tests/cpp/host_signature_leaves.cpp: g++, the C ABI only): the exported
leaf recording and the raw bytes of four slots — three signed, one unflagged — go glp_ed25519_leaf_inputs -> glp_witness_eval_device ->
glp_witness_place_batch -> glp_plonk_prove_batch, and the four leaf proofs equal, byte for byte, the ones the Python Map step makes for the same
slots (device_witness, groups of four).  6 queries, 4 PoW bits."""
import hashlib
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from conftest import ROOT, poseidon_consts  # noqa: E402
import __graft_entry__ as graft  # noqa: E402

NQ, PW = 6, 4


def _mod(name):
    graft.load_package()
    return importlib.import_module(graft.PKG_NAME + name)


@pytest.mark.gpu
def test_cpp_host_proves_the_signature_leaves(pkg, prover, tmp_path):
    sm, ec = _mod(".signature_mr"), _mod(".ed25519_circuit")
    consts = poseidon_consts("small")
    prover.set_poseidon_constants(*consts)
    sigs = sm.SignatureSetMapReduce(prover, consts, msg_len=48, hash_offset=8, fan_in=2, num_queries=NQ, pow_bits=PW, device_witness=True,
                                    device_witness_chunk=4, prove_batch=4)
    try:
        sigs._record_leaf()
        block = hashlib.sha256(b"a block").digest()
        flags = [True, True, False, True]
        msgs = [sigs.vote_bytes(block, i) for i in range(4)]
        keys = [ec.keypair_and_sign(hashlib.sha256(b"seed %d" % i).digest(), m) for i, m in enumerate(msgs)]
        pubs, sg = [k[0] for k in keys], [k[1] if f else None for k, f in zip(keys, flags)]
        leaves = sigs._map(sigs._slots(pubs, sg, msgs, flags), 0, 4)                 # the Python Map step: witness_inputs on the host
        sigs.leaf_program.export_raw(str(tmp_path / "leaf"))
        layout = sigs._input_layout()
        with open(tmp_path / "slots.bin", "wb") as f:
            f.write(np.array([layout.form, layout.msg_len_min, layout.msg_len_max, layout.split_scalars, 4, 48], dtype="<u4").tobytes())
            f.write(b"".join(pubs) + b"".join(s if s is not None else bytes(64) for s in sg) + b"".join(msgs))
            f.write(np.array([48] * 4, dtype="<u4").tobytes() + bytes(int(x) for x in flags) + b"".join(ec.dummy_signature(48)))
        np.concatenate([np.asarray(a, dtype=np.uint64) for a in consts]).astype("<u8").tofile(str(tmp_path / "pc.bin"))
        exe = tmp_path / "host_signature_leaves"
        libdir = os.path.dirname(pkg.LIB_PATH)
        subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "host_signature_leaves.cpp"), "-o", str(exe), "-L", libdir, "-lglprover", "-pthread",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
        r = subprocess.run([str(exe), str(tmp_path / "pc.bin"), str(NQ), str(PW), str(tmp_path / "leaf"), str(tmp_path / "slots.bin"),
                            str(tmp_path / "proof")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip().endswith("OK"), r.stdout
        assert "input launches 2 syncs 1" in r.stdout and "status 0 0 0 0" in r.stdout, r.stdout
        lines = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines() if " " in ln)
        assert int(lines["key0"]) == int(sigs.leaf_circuit.cap()[0])
        for i in range(4):
            proof = (tmp_path / f"proof{i}.bin").read_bytes()
            assert proof == leaves[i], f"leaf {i} is not the Map step's proof"
            assert [int(v) for v in lines[f"public{i}"].split()] == [int(v) for v in pkg.proof_public_inputs(proof)]
    finally:
        sigs.free()
