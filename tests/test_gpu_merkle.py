"""gfx950 SHA-256 merkle kernels (ops._gpumerkle) vs hashlib - needs a real MI355X.

The reference is an independent recursive tree over hashlib; equality is bit-exact.
"""
from __future__ import annotations

import hashlib
import os

import pytest

pytestmark = pytest.mark.gpu

LEAF = 16384


def sha256(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def ref_root(nodes):
    if len(nodes) == 1:
        return nodes[0]
    h = len(nodes) // 2
    return sha256(ref_root(nodes[:h]) + ref_root(nodes[h:]))


def pow2(n: int) -> int:
    p = 1
    while p < n:
        p *= 2
    return p


def ref_leaves(data: bytes):
    return [sha256(data[i:i + LEAF]) for i in range(0, len(data), LEAF)]


def ref_tree(data: bytes, piece_len: int):
    leaves = ref_leaves(data)
    if len(data) <= piece_len:
        return b"", ref_root(leaves + [bytes(32)] * (pow2(len(leaves)) - len(leaves)))
    per = piece_len // LEAF
    layer = []
    for i in range(0, len(leaves), per):
        grp = leaves[i:i + per]
        layer.append(ref_root(grp + [bytes(32)] * (per - len(grp))))
    pad = ref_root([bytes(32)] * per)
    return b"".join(layer), ref_root(layer + [pad] * (pow2(len(layer)) - len(layer)))


def blob(n: int, seed: int = 1) -> bytes:
    out = bytearray()
    h = hashlib.sha256(b"gpu-seed%d" % seed).digest()
    while len(out) < n:
        h = hashlib.sha256(h).digest()
        out += h * 16
    return bytes(out[:n])


@pytest.fixture(scope="module")
def gm():
    from downloader_amd.ops import gpu_available, gpumerkle
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    assert gpumerkle().device_count() > 0
    assert "gfx950" in gpumerkle().arch()
    return gpumerkle()


@pytest.fixture(scope="module")
def mh(gm):
    return gm.MerkleHasher(0, 4 << 20, 4)


@pytest.mark.parametrize("n", [64 * LEAF, 65 * LEAF + 1, 257 * LEAF, 1,
                               3 * LEAF + 55, 3 * LEAF + 56, 3 * LEAF + 63, 3 * LEAF + 64,
                               3 * LEAF + 16383])
def test_leaf_hashes_match_hashlib(mh, n):
    data = blob(n, n)
    assert mh.leaf_hashes(data) == b"".join(ref_leaves(data))
    assert mh.leaf_hashes(memoryview(bytearray(data))) == b"".join(ref_leaves(data))


@pytest.mark.parametrize("k", [1, 2, 3, 64, 65, 255, 256, 257])
def test_reduce_layer_matches_hashlib(mh, k):
    hashes = blob(32 * k, 1000 + k)
    pad = blob(32, 77)
    full = hashes + (pad if k % 2 else b"")
    want = b"".join(sha256(full[i:i + 64]) for i in range(0, len(full), 64))
    assert mh.reduce_layer(hashes, pad) == want
    assert len(want) == 32 * ((k + 1) // 2)


def test_pad_hash_levels(mh):
    assert mh.pad_hash(0) == bytes(32)
    assert mh.pad_hash(1).hex() == \
        "f5a5fd42d16a20302798ef6ed309979b43003d2320d9f0e8ea9831a92759fb4b"
    assert mh.pad_hash(6) == ref_root([bytes(32)] * 64)


@pytest.mark.parametrize("piece_len", [16384, 65536])
@pytest.mark.parametrize("length", [1, 16385, 3 * 16384, 5 * 16384 + 7])
def test_hash_buffer_and_hash_file_match_the_recursive_reference(mh, tmp_path, length, piece_len):
    data = blob(length, length + piece_len)
    want = ref_tree(data, piece_len)
    assert mh.hash_buffer(data, piece_len) == want
    p = tmp_path / "f.bin"
    p.write_bytes(data)
    assert mh.hash_file(str(p), length, piece_len) == want


def test_several_batches_and_a_partial_last_one(gm, tmp_path):
    """9.5 MiB + 7 in 256 KiB pieces through 1 MiB slots: ten batches of four pieces, the
    last one of three pieces with a short last piece."""
    h = gm.MerkleHasher(0, 1 << 20, 4)
    n = (19 << 19) + 7
    data = blob(n, 5)
    want = ref_tree(data, 256 << 10)
    assert len(want[0]) == 32 * 39
    assert h.hash_buffer(data, 256 << 10) == want
    p = tmp_path / "big.bin"
    p.write_bytes(data)
    assert h.hash_file(str(p), n, 256 << 10) == want


def test_file_of_exactly_two_batches(gm, tmp_path):
    """The last lane of each batch ends exactly at the end of the device buffer."""
    h = gm.MerkleHasher(0, 1 << 20, 2)
    data = blob(2 << 20, 6)
    for plen in (16384, 1 << 20):
        want = ref_tree(data, plen)
        assert h.hash_buffer(data, plen) == want
        p = tmp_path / "two.bin"
        p.write_bytes(data)
        assert h.hash_file(str(p), len(data), plen) == want


def flip(path, offset: int) -> None:
    with open(path, "r+b") as f:
        f.seek(offset)
        b = f.read(1)
        f.seek(offset)
        f.write(bytes([b[0] ^ 0x01]))


def test_verify_file(gm, tmp_path):
    h = gm.MerkleHasher(0, 1 << 20, 4)      # 256 KiB pieces: four to a batch, three batches
    plen = 256 << 10
    n = 9 * plen + 1000                     # ten pieces, a short last one
    data = blob(n, 8)
    layer, _root = ref_tree(data, plen)
    p = tmp_path / "v.bin"
    p.write_bytes(data)
    assert h.verify_file(str(p), n, plen, layer) == b"\x01" * 10
    flip(p, 5 * plen + 4321)
    assert h.verify_file(str(p), n, plen, layer) == b"\x01" * 5 + b"\x00" + b"\x01" * 4
    flip(p, 5 * plen + 4321)
    flip(p, n - 1)
    assert h.verify_file(str(p), n, plen, layer) == b"\x01" * 9 + b"\x00"
    flip(p, n - 1)
    with open(p, "r+b") as f:               # cut inside piece 6
        f.truncate(6 * plen + 99)
    assert h.verify_file(str(p), n, plen, layer) == b"\x01" * 6 + b"\x00" * 4
    os.unlink(p)
    assert h.verify_file(str(p), n, plen, layer) == bytes(10)
    # a file no larger than a piece is checked against its root: exactly one byte
    small = blob(100000, 9)
    q = tmp_path / "s.bin"
    q.write_bytes(small)
    root = ref_tree(small, plen)[1]
    assert h.verify_file(str(q), len(small), plen, root) == b"\x01"
    flip(q, 99999)
    assert h.verify_file(str(q), len(small), plen, root) == b"\x00"
    with open(q, "r+b") as f:
        f.truncate(50000)
    assert h.verify_file(str(q), len(small), plen, root) == b"\x00"


def test_argument_errors(mh, tmp_path):
    data = blob(5 * LEAF, 10)
    p = tmp_path / "a.bin"
    p.write_bytes(data)
    for bad in (24576, 8192, 8 << 20):      # no power of two, below 16 KiB, above batch_bytes
        with pytest.raises(ValueError):
            mh.hash_buffer(data, bad)
        with pytest.raises(ValueError):
            mh.hash_file(str(p), len(data), bad)
        with pytest.raises(ValueError):
            mh.verify_file(str(p), len(data), bad, bytes(32))
    with pytest.raises(ValueError):
        mh.verify_file(str(p), len(data), 16384, bytes(32 * 4))     # five pieces
    with pytest.raises(ValueError):
        mh.verify_file(str(p), len(data), 1 << 20, bytes(64))       # a root is 32 bytes
    stepped = memoryview(bytearray(data))[::2]
    with pytest.raises(ValueError):
        mh.leaf_hashes(stepped)
    with pytest.raises(ValueError):
        mh.hash_buffer(stepped, 16384)
    with pytest.raises(ValueError):
        mh.reduce_layer(bytes(33), bytes(32))
    with pytest.raises(ValueError):
        mh.reduce_layer(bytes(64), bytes(31))


def test_file_tree_gpu_backend_equals_cpu(gm, tmp_path):
    from downloader_amd.torrent import merkle
    n = (3 << 20) + 5
    data = blob(n, 11)
    p = tmp_path / "t.bin"
    p.write_bytes(data)
    cpu = merkle.file_tree(str(p), n, 65536, backend="cpu")
    assert merkle.file_tree(str(p), n, 65536, backend="gpu") == cpu
    assert merkle.verify_file(str(p), n, 65536, cpu[0], backend="gpu") == b"\x01" * 49


def test_hash_pieces_sha256_leaf_route(gm):
    from downloader_amd.ops import hashing
    data = blob(7 * LEAF + 123, 12)
    cpu = hashing.hash_pieces(data, 16384, "sha256", backend="cpu")
    assert hashing.hash_pieces(data, 16384, "sha256", backend="gpu") == cpu
    with pytest.raises(ValueError):         # every other SHA-256 shape is still refused
        hashing.hash_pieces(data, 32768, "sha256", backend="gpu")
