"""Host-side mirror of the circuit-level witness logic either side of the prover hot path
(SURVEY.md §1b layers L4/L5, §8a rows a9/a10; BASELINE configs[0]): what a ``Circuit::define`` of
CombinedStep / CombinedSkip / DataCommitment computes as WITNESS — validator-set hashing, signature
verification, voting-power thresholds, the data-commitment Merkle root, and the packing of the public
values — driven through the C ABI (SHA-256 Merkle and Ed25519 kernels).

Everything here restates PUBLIC formats from memory, because the reference mount is empty
(`/root/reference/.gitignore:1`, `changelog.md:1-2`): each item is tagged

  [SPEC]      a published definition this follows (RFC 6962 Merkle trees, RFC 8032 Ed25519, protobuf
              wire format, Solidity ABI encoding) and that the tests pin with independent Python code;
  [RECALLED]  how upstream (tendermint / blobstreamx / tendermintx) uses it, recalled and UNVERIFIED —
              never a parity claim.

No CPU fallback: every hash and signature check below runs in the HIP kernels of libglprover.so.
"""
import collections
import struct

import numpy as np

# ---- encodings ---------------------------------------------------------------------------------


def encode_varint(u: int) -> bytes:
    """[SPEC] protobuf base-128 varint of a non-negative integer"""
    if u < 0:
        raise ValueError("negative varint")
    out = bytearray()
    while True:
        b = u & 0x7F
        u >>= 7
        if u:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def encode_validator(pubkey: bytes, voting_power: int) -> bytes:
    """[SPEC] protobuf wire format of  message SimpleValidator { PublicKey pub_key = 1; int64 voting_power = 2; }
    with  message PublicKey { oneof sum { bytes ed25519 = 1; } }.
    [RECALLED] this is the Merkle leaf of Tendermint's ValidatorSet.Hash()."""
    if len(pubkey) != 32:
        raise ValueError("ed25519 public key must be 32 bytes")
    if not 0 <= voting_power < 2**63:
        raise ValueError("voting power out of int64 range")
    inner = b"\x0a" + encode_varint(32) + pubkey                     # PublicKey.ed25519
    out = b"\x0a" + encode_varint(len(inner)) + inner                # SimpleValidator.pub_key
    if voting_power:
        out += b"\x10" + encode_varint(voting_power)                 # SimpleValidator.voting_power (omitted when 0)
    return out


def encode_data_root_tuple(height: int, data_root: bytes) -> bytes:
    """[SPEC] Solidity abi.encode(uint256 height, bytes32 dataRoot): two 32-byte words.
    [RECALLED] the leaf of Blobstream's data commitment (DataRootTuple)."""
    if len(data_root) != 32 or not 0 <= height < 2**256:
        raise ValueError("bad data root tuple")
    return height.to_bytes(32, "big") + data_root


def canonical_vote_sign_bytes(chain_id, height, round, block_hash, part_total, part_hash, seconds, nanos, vote_type=2) -> bytes:
    """[SPEC] recalled, unpinned: the sign-bytes of a Tendermint / CometBFT vote — protobuf ``CanonicalVote``, length-delimited (no upstream
    source is in the mount: the layout below is restated from the public definition and pinned only by this repository's own tests).

        varint(len(body)) ‖ body
        body = 08 tt                      type (02 precommit, 01 prevote)
               11 <height: 8 bytes LE>    sfixed64
               19 <round: 8 bytes LE>     sfixed64, only when round != 0
               22 LL  0a 20 <hash:32>  12 MM ( 08 varint(part_total)  12 20 <part_hash:32> )        CanonicalBlockID
               2a NN  08 varint(seconds) [10 varint(nanos) when nanos != 0]                          google.protobuf.Timestamp
               32 KK <chain_id>

    Fields in number order; zero scalars and empty strings are omitted (proto3), embedded messages are always written.  Every validator signs
    its OWN timestamp, so the votes of one commit differ in length by the nanos varint (absent, or 1 to 5 bytes)."""
    chain = chain_id.encode() if isinstance(chain_id, str) else bytes(chain_id)
    block_hash, part_hash = bytes(block_hash), bytes(part_hash)
    if len(block_hash) != 32 or len(part_hash) != 32:
        raise ValueError("block hash and part-set hash are 32 bytes")
    if height <= 0 or height >= 1 << 63 or not 0 <= round < 1 << 63:
        raise ValueError("height must be positive, round non-negative (sfixed64)")
    if seconds < 0 or nanos < 0 or nanos >= 10**9:
        raise ValueError("timestamp out of range: seconds >= 0, 0 <= nanos < 10^9")
    if vote_type not in (1, 2) or part_total < 0:
        raise ValueError("vote type is 1 (prevote) or 2 (precommit); part total is non-negative")
    psh = (b"\x08" + encode_varint(part_total) if part_total else b"") + b"\x12\x20" + part_hash
    block_id = b"\x0a\x20" + block_hash + b"\x12" + encode_varint(len(psh)) + psh
    stamp = (b"\x08" + encode_varint(seconds) if seconds else b"") + (b"\x10" + encode_varint(nanos) if nanos else b"")
    body = b"\x08" + bytes([vote_type]) + b"\x11" + struct.pack("<q", height)
    if round:
        body += b"\x19" + struct.pack("<q", round)
    body += b"\x22" + encode_varint(len(block_id)) + block_id + b"\x2a" + encode_varint(len(stamp)) + stamp
    if chain:
        body += b"\x32" + encode_varint(len(chain)) + chain
    return encode_varint(len(body)) + body


class VoteFormat:
    """What a signature circuit fixes about the canonical votes it accepts: whether the round field is present, and the window
    [min_len, max_len] of TOTAL sign-bytes lengths (length prefix included).  Derived: ``prefix_len`` (bytes of the length prefix), ``base`` (offset
    of the block id's tag 22) and ``hash_offset`` (offset of the 32 block-hash bytes).
    STATED LIMITS (ValueError otherwise): the window must not straddle the 1-byte / 2-byte length prefix (max_len <= 128, or min_len >= 130 —
    a total of 129 does not exist), and 48 <= min_len, max_len <= 175: exactly there SHA-512 of R ‖ A ‖ M is two blocks for every length of the
    window, which is what lets one circuit hash all of them."""
    __slots__ = ("round_present", "min_len", "max_len")

    def __init__(self, round_present, min_len, max_len):
        self.round_present, self.min_len, self.max_len = bool(round_present), int(min_len), int(max_len)
        if self.min_len > self.max_len:
            raise ValueError("empty length window")
        if not (self.max_len <= 128 or self.min_len >= 130):
            raise ValueError("the length window straddles the 1-byte / 2-byte length prefix: split it into two formats")
        if self.min_len < 48 or self.max_len > 175:
            raise ValueError("the length window leaves [48, 175]: SHA-512 of R || A || M is no longer two blocks for every length")
        if self.hash_offset + 32 > self.min_len:
            raise ValueError("the shortest vote of the window cannot hold the block hash")

    @property
    def prefix_len(self):
        return 1 if self.max_len <= 128 else 2

    @property
    def base(self):
        return self.prefix_len + 11 + (9 if self.round_present else 0)

    @property
    def hash_offset(self):
        return self.base + 4

    @classmethod
    def for_commit(cls, chain_id, round, seconds_bytes=5, part_total_bytes=1):
        """the format of the votes of ONE commit: chain id and round are the commit's, the seconds varint has seconds_bytes bytes (5 for any
        date from 1978 to 3058), the part total part_total_bytes; the window spans the nanos field from omitted to 5 varint bytes"""
        chain = chain_id.encode() if isinstance(chain_id, str) else bytes(chain_id)
        psh = 1 + part_total_bytes + 34
        block_id = 34 + 2 + psh
        if block_id >= 128 or len(chain) >= 128 or not 1 <= seconds_bytes <= 9 or part_total_bytes < 1:
            raise ValueError("field lengths outside the one-byte length forms this layout assumes")
        body = 2 + 9 + (9 if round else 0) + 2 + block_id + 2 + (1 + seconds_bytes) + (2 + len(chain) if chain else 0)
        lo, hi = body, body + 6
        return cls(bool(round), lo + len(encode_varint(lo)), hi + len(encode_varint(hi)))

    def __eq__(self, other):
        return isinstance(other, VoteFormat) and self.as_tuple() == other.as_tuple()

    def __hash__(self):
        return hash(self.as_tuple())

    def as_tuple(self):
        return (self.round_present, self.min_len, self.max_len)

    def __repr__(self):
        return f"VoteFormat(round_present={self.round_present}, min_len={self.min_len}, max_len={self.max_len})"


# ---- hashing witnesses (GPU) -------------------------------------------------------------------


def validator_set_hash(prover, pubkeys, voting_powers) -> bytes:
    """Merkle root ([SPEC] RFC 6962 tree with 0x00 / 0x01 prefixes, as Tendermint's simple Merkle tree) of the
    encoded validators — BASELINE configs[0]'s "validator-Merkle witness"."""
    return prover.tm_merkle_root_var([encode_validator(k, p) for k, p in zip(pubkeys, voting_powers)])


def data_commitment(prover, heights, data_roots) -> bytes:
    """[RECALLED] Blobstream data commitment of a block range: the same Merkle tree over
    abi.encode(height, dataRoot) for every block of the range (DataCommitmentCircuit's witness)."""
    leaves = b"".join(encode_data_root_tuple(h, r) for h, r in zip(heights, data_roots))
    return prover.tm_merkle_root(leaves, 64)


# ---- inclusion proofs (GPU) --------------------------------------------------------------------

# BUILD-DEFINED: [RECALLED] Tendermint's crypto/merkle.Proof{Total, Index, LeafHash, Aunts}, restated from memory and unpinned — the aunts are the
# sibling hashes bottom-up (nearest the leaf first), 32 bytes each; an odd last node of a level is promoted and contributes no aunt there.
InclusionProof = collections.namedtuple("InclusionProof", "total index leaf_hash aunts")


def _forest_proofs(prover, trees, queries):
    forest = prover.tm_forest(trees)
    try:
        return forest.roots(), [InclusionProof(*p) for p in forest.proofs(queries)]
    finally:
        forest.free()


def data_root_inclusion_proofs(prover, heights, data_roots, indices=None):
    """(commitment, [InclusionProof]) of a block range: the data commitment (the root data_commitment gives) and the audit path of every
    DataRootTuple of the range, or of the tuples `indices` — ONE forest build and one path launch on the device (glp_tm_forest_*).
    [RECALLED] what Blobstream's verifyAttestation checks against the commitment."""
    leaves = [encode_data_root_tuple(h, r) for h, r in zip(heights, data_roots)]
    roots, proofs = _forest_proofs(prover, [leaves], None if indices is None else [(0, int(i)) for i in indices])
    return roots[0], proofs


def verify_data_root_inclusions(prover, commitment, heights, data_roots, proofs):
    """the list form: status int32[n] (TM_INCLUSION_OK = 0 / BAD_SHAPE / BAD_ROOT) of proofs[k] for the tuple (heights[k], data_roots[k]) against
    the commitment alone, in one launch.  The tuple's BYTES are hashed on the device; the proof's leaf_hash is not trusted."""
    leaves = [encode_data_root_tuple(h, r) for h, r in zip(heights, data_roots)]
    return prover.tm_verify_inclusion_batch([bytes(commitment)], proofs, leaves)


def verify_data_root_inclusion(prover, commitment, height, data_root, proof) -> bool:
    """True when `proof` places the tuple (height, data_root) inside `commitment`"""
    return int(verify_data_root_inclusions(prover, commitment, [height], [data_root], [proof])[0]) == 0


def validator_inclusion_proofs(prover, pubkeys, powers, indices=None):
    """(validators hash, [InclusionProof]) of a validator set: membership proofs of every validator, or of `indices` (leaves of differing lengths)"""
    leaves = [encode_validator(k, p) for k, p in zip(pubkeys, powers)]
    roots, proofs = _forest_proofs(prover, [leaves], None if indices is None else [(0, int(i)) for i in indices])
    return roots[0], proofs


def header_field_proofs(prover, headers_fields, field_index):
    """([header hash], [InclusionProof]) of B headers in ONE forest call: headers_fields[b] = the 14 field encodings of header b; proof b places
    field `field_index` (6 = data_hash, 4 = last_block_id) inside header b's hash"""
    return _forest_proofs(prover, [[bytes(x) for x in f] for f in headers_fields], [(b, int(field_index)) for b in range(len(headers_fields))])


# ---- signatures and voting power ---------------------------------------------------------------


def verify_signatures(prover, pubkeys, signatures, sign_bytes):
    """[SPEC] RFC 8032 Ed25519 verification of signatures[i] by pubkeys[i] over sign_bytes[i], all on the GPU
    (glp_ed25519_witness: decoded points, k = SHA-512(R || A || M) mod L, [S]B and [k]A).  Entries whose
    signature is None count as absent.  Returns (valid flags, witness records [n][37] u64)."""
    n = len(pubkeys)
    present = [i for i in range(n) if signatures[i] is not None]
    valid = np.zeros(n, dtype=bool)
    rec = np.zeros((n, 37), dtype=np.uint64)
    if present:
        out = prover.ed25519_witness([pubkeys[i] for i in present], [signatures[i] for i in present], [sign_bytes[i] for i in present])
        for j, i in enumerate(present):
            rec[i] = out[j]
            valid[i] = bool(out[j][0])
    return valid, rec


def verify_signers(prover, poseidon_consts, signer_digest, pubkeys, signed, signatures, sign_bytes):
    """The hybrid half of a commit check whose proof does NOT constrain Ed25519 (gadgets.step_circuit / skip_circuit): the proof's public inputs
    carry a digest of (target validator keys, signed flags); the consumer, who holds the keys, the flags and the signatures, checks that
      1. the digest of (pubkeys, signed) IS the proof's signer digest — the proof's power rules were about exactly these flags, and
      2. every FLAGGED validator's signature verifies ([SPEC] RFC 8032, on the GPU witness kernel) over its sign bytes.
    Unflagged validators need no signature.  sign_bytes[i] is validator i's canonical vote: the consumer BUILDS it around the target header hash the
    proof exposes (block id, height, round, its own timestamp, chain id — [RECALLED] CanonicalVote), otherwise the signatures are about something
    else; this function does not know the vote format and takes the bytes as given.  Returns True / False."""
    import importlib
    gd = importlib.import_module(__package__ + ".gadgets")
    if [int(v) for v in signer_digest] != gd.signer_digest_host(poseidon_consts, pubkeys, signed):
        return False
    flagged = [i for i, sg in enumerate(signed) if sg]
    if any(signatures[i] is None for i in flagged):
        return False
    valid, _ = verify_signatures(prover, [pubkeys[i] for i in flagged], [signatures[i] for i in flagged], [sign_bytes[i] for i in flagged])
    return bool(all(valid))


def voting_power_check(voting_powers, signed, numerator, denominator):
    """signed_power * denominator > total_power * numerator, in exact integers ([RECALLED] Tendermint's
    "more than 2/3" commit rule and the light client's "more than 1/3 of the trusted set" skipping rule).
    Returns (signed_power, total_power, ok)."""
    total = int(sum(int(p) for p in voting_powers))
    got = int(sum(int(p) for p, s in zip(voting_powers, signed) if s))
    return got, total, got * denominator > total * numerator


def skip_witness(prover, trusted_pubkeys, trusted_powers, target_pubkeys, target_powers, target_signatures, target_sign_bytes):
    """The witness of a light-client skip ([RECALLED] tendermintx verify_skip, the core of CombinedSkipCircuit):
      1. the target header's validators hash to `validators_hash` (committed in that header),
      2. validators holding > 2/3 of the target set's power signed the target header,
      3. signers that are also in the trusted set hold > 1/3 of the TRUSTED set's power.
    target_signatures[i] is validator i's signature over target_sign_bytes[i] (its canonical vote; each
    validator signs its own timestamp) or None."""
    valid, rec = verify_signatures(prover, target_pubkeys, target_signatures, target_sign_bytes)
    signed_power, total_power, two_thirds = voting_power_check(target_powers, valid, 2, 3)
    trusted = {bytes(k): int(p) for k, p in zip(trusted_pubkeys, trusted_powers)}
    overlap = sum(trusted.get(bytes(k), 0) for k, v in zip(target_pubkeys, valid) if v)
    trusted_total = sum(trusted.values())
    return {
        "validators_hash": validator_set_hash(prover, target_pubkeys, target_powers),
        "trusted_validators_hash": validator_set_hash(prover, trusted_pubkeys, trusted_powers),
        "signature_valid": valid,
        "signature_witness": rec,
        "signed_power": signed_power,
        "total_power": total_power,
        "two_thirds_signed": two_thirds,
        "trusted_power_signed": overlap,
        "trusted_total_power": trusted_total,
        "one_third_of_trusted_signed": overlap * 3 > trusted_total,
        "accept": bool(two_thirds and overlap * 3 > trusted_total),
    }


# ---- public values ([RECALLED] plonky2x evm_read / evm_write: big-endian, tightly packed) ------


def pack_skip_inputs(trusted_block: int, trusted_header_hash: bytes, target_block: int) -> bytes:
    """uint64 ‖ bytes32 ‖ uint64 as abi.encodePacked"""
    if len(trusted_header_hash) != 32:
        raise ValueError("header hash must be 32 bytes")
    return struct.pack(">Q", trusted_block) + trusted_header_hash + struct.pack(">Q", target_block)


def pack_step_inputs(trusted_block: int, trusted_header_hash: bytes) -> bytes:
    if len(trusted_header_hash) != 32:
        raise ValueError("header hash must be 32 bytes")
    return struct.pack(">Q", trusted_block) + trusted_header_hash


def pack_outputs(target_header_hash: bytes, data_commitment_root: bytes) -> bytes:
    """bytes32 ‖ bytes32"""
    if len(target_header_hash) != 32 or len(data_commitment_root) != 32:
        raise ValueError("outputs are two bytes32")
    return target_header_hash + data_commitment_root


def unpack_skip_inputs(b: bytes):
    if len(b) != 48:
        raise ValueError("skip inputs are 48 bytes")
    return struct.unpack(">Q", b[:8])[0], b[8:40], struct.unpack(">Q", b[40:])[0]


def public_words(packed: bytes):
    """the packed public values as field elements for the circuit's public-input rows: big-endian 32-bit words, one per element
    (each < 2^32 < p, so the map bytes -> elements is injective).  BUILD-DEFINED: how plonky2x maps evm_read/evm_write bytes to
    public-input targets is not in the mount ([RECALLED]: one target per byte); the verifier only needs both sides to agree."""
    if len(packed) % 4:
        raise ValueError("public values must be a whole number of 32-bit words")
    return [int.from_bytes(packed[i:i + 4], "big") for i in range(0, len(packed), 4)]
