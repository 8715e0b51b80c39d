"""BitTorrent v2 (BEP 52) merkle trees: the tree rules, a CPU backend on the native hashing
module and the dispatch to the gfx950 module (``ops._gpumerkle``, csrc/gpu_sha256_merkle.hip).

Tree rules
  * A leaf is the SHA-256 of one 16 KiB block; the last leaf of a file is hashed at its true
    length. A missing leaf is 32 zero bytes.
  * ``pad_hash(0)`` is 32 zero bytes and ``pad_hash(k + 1) = sha256(pad_hash(k) * 2)``: the
    hash of an all-missing subtree of 2**k leaves.
  * A file no larger than a piece has no piece layer; its ``pieces root`` is the root over its
    leaves padded with zero leaves to the next power of two (not up to the piece size).
  * A larger file's piece layer is the ceil(length / piece_len) nodes that each cover
    ``piece_len`` bytes (the last piece's subtree completed with zero leaves); its root is taken
    over that layer padded to a power of two with ``pad_hash(log2(piece_len / 16384))``.
  * An empty file has no root and no pieces.

``backend``: ``cpu``, ``gpu`` (RuntimeError without a device) or ``auto``. For a recheck of at
least ``hashing.GPU_MIN_BYTES``, ``auto`` is the device when one is there: on the MI355X box a
4 GiB recheck of 1 MiB pieces ran at 34.7 GB/s through the device against 8.5 GB/s on 16 host
threads (docs/PERFORMANCE.md, "BitTorrent v2 recheck"), far beyond the 10 % margin the rule
asks for. Creation was not measured: there ``auto`` stays on the host.

``verify_files`` / ``hash_files`` take a whole torrent's files. On the device they are one
``MerkleHasher`` call in which pieces of many files share a batch: 40.9 against 32.7 GB/s file
by file on that recheck, and 38.2 against 3.1 GB/s with 4,096 small files added to it
(docs/PERFORMANCE.md, "Batched across files").
"""
from __future__ import annotations

import os
import threading
from typing import List, Tuple

from ..ops import gpu_available, gpumerkle, hashing, native

LEAF = 16384
ZERO = bytes(32)

# The measured rule for ``auto``: the device for v2 rechecks of at least hashing.GPU_MIN_BYTES
# only if its end-to-end rate beats the host's by more than 10 % (the run-to-run spread of the
# host path). It did, 4.1 x (module docstring).
AUTO_USES_GPU = True

_pads: List[bytes] = [ZERO]
_pads_lock = threading.Lock()


def pad_hash(level: int) -> bytes:
    """Hash of an all-missing subtree of ``2 ** level`` leaves."""
    if level < 0:
        raise ValueError("pad_hash: negative level")
    with _pads_lock:
        while len(_pads) <= level:
            _pads.append(native().digest("sha256", _pads[-1] * 2))
        return _pads[level]


def check_piece_length(piece_len: int) -> int:
    """log2(piece_len / 16384) of a valid v2 piece length; ValueError otherwise."""
    from .metainfo import MAX_PIECE_LENGTH
    if not isinstance(piece_len, int) or piece_len < LEAF or piece_len & (piece_len - 1):
        raise ValueError(f"piece length {piece_len!r} is not a power of two of at least {LEAF}")
    if piece_len > MAX_PIECE_LENGTH:
        raise ValueError(f"piece length {piece_len} above {MAX_PIECE_LENGTH}")
    return (piece_len // LEAF).bit_length() - 1


def pow2_ceil(n: int) -> int:
    return 1 << max(0, n - 1).bit_length()


def num_pieces(length: int, piece_len: int) -> int:
    return (length + piece_len - 1) // piece_len


def choose_backend(requested: str, total_bytes: int = 0, recheck: bool = False) -> str:
    """``auto`` picks the device only for a recheck (``verify_file``) of ``total_bytes``."""
    if requested == "cpu":
        return "cpu"
    if requested == "gpu":
        if not gpu_available():
            raise RuntimeError("backend=gpu but no HIP device is available")
        return "gpu"
    if requested != "auto":
        raise ValueError(f"unknown backend {requested!r}")
    if recheck and AUTO_USES_GPU and total_bytes >= hashing.GPU_MIN_BYTES and gpu_available():
        return "gpu"
    return "cpu"


_hasher = None
_hasher_lock = threading.Lock()      # creation
_call_lock = threading.Lock()        # one MerkleHasher owns two slots and two streams


def gpu_hasher():
    """The process's ``MerkleHasher`` (created on first use, on the worker's device)."""
    global _hasher
    with _hasher_lock:
        if _hasher is None:
            _hasher = gpumerkle().MerkleHasher(hashing.gpu_device(), 256 << 20, 8)
        return _hasher


def leaf_hashes(data, backend: str = "cpu", threads: int = 0) -> bytes:
    """32 bytes per 16 KiB block of a contiguous buffer."""
    if choose_backend(backend, memoryview(data).nbytes) == "gpu":
        h = gpu_hasher()
        with _call_lock:
            return h.leaf_hashes(data)
    return native().hash_pieces("sha256", data, LEAF, threads)


def reduce_to(hashes: bytes, width: int, level: int = 0, threads: int = 0) -> bytes:
    """Merge every ``width`` (a power of two) nodes of a layer at tree level ``level`` into
    their common ancestor: ceil(k / width) x 32 bytes. A group that is not full is completed
    with missing subtrees, one ``pad_hash`` of the level at hand whenever a level is odd."""
    if width < 1 or width & (width - 1):
        raise ValueError("width must be a power of two")
    if len(hashes) % 32:
        raise ValueError("a layer is a whole number of 32-byte hashes")
    n = native()
    while width > 1 and hashes:
        if (len(hashes) // 32) & 1:
            hashes = hashes + pad_hash(level)
        hashes = n.hash_pieces("sha256", hashes, 64, threads)
        level += 1
        width >>= 1
    return hashes


def tree_from_leaves(leaves: bytes, length: int, piece_len: int,
                     threads: int = 0) -> Tuple[bytes, bytes]:
    """(piece_layer, root) from a file's leaf layer."""
    k = check_piece_length(piece_len)
    if length <= piece_len:
        return b"", reduce_to(leaves, pow2_ceil(len(leaves) // 32), 0, threads)
    layer = reduce_to(leaves, piece_len // LEAF, 0, threads)
    return layer, layer_root(layer, k, threads)


def layer_root(layer: bytes, level: int, threads: int = 0) -> bytes:
    """``pieces root`` over a piece layer whose nodes sit at tree level ``level``."""
    return reduce_to(layer, pow2_ceil(len(layer) // 32), level, threads)


def file_tree(path: str, length: int, piece_len: int, backend: str = "cpu",
              threads: int = 0) -> Tuple[bytes, bytes]:
    """(piece_layer, pieces root) of the first ``length`` bytes of ``path``; ``(b"", b"")`` for
    an empty file, an empty layer for a file no larger than a piece."""
    check_piece_length(piece_len)
    be = choose_backend(backend, length)
    if length <= 0:
        return b"", b""
    if be == "gpu":
        h = gpu_hasher()
        with _call_lock:
            layer, root = h.hash_file(str(path), int(length), int(piece_len))
        return layer, root
    leaves = native().hash_storage_pieces([(str(path), int(length))], LEAF, "sha256", threads)
    return tree_from_leaves(leaves, length, piece_len, threads)


def verify_file(path: str, length: int, piece_len: int, expected: bytes, backend: str = "cpu",
                threads: int = 0) -> bytes:
    """One byte per piece (1 = good). ``expected`` is the piece layer for a file larger than a
    piece and the 32-byte ``pieces root`` otherwise (exactly one byte comes back then). Pieces
    that a missing or short file does not cover are 0."""
    check_piece_length(piece_len)
    if length <= 0:
        raise ValueError("an empty file has no pieces")
    small = length <= piece_len
    np_ = 1 if small else num_pieces(length, piece_len)
    if len(expected) != 32 * np_:
        raise ValueError(f"expected is {len(expected)} bytes, want {32 * np_}")
    if choose_backend(backend, length, recheck=True) == "gpu":
        h = gpu_hasher()
        with _call_lock:
            return h.verify_file(str(path), int(length), int(piece_len), bytes(expected))
    try:
        have = min(os.path.getsize(path), length)
    except OSError:
        have = 0
    if have < length:                      # only whole pieces that the file covers are hashed
        if small or have < piece_len:
            return bytes(np_)
        have -= have % piece_len
    leaves = native().hash_storage_pieces([(str(path), int(have))], LEAF, "sha256", threads)
    if small:
        return bytes([reduce_to(leaves, pow2_ceil(len(leaves) // 32), 0, threads) == expected])
    layer = reduce_to(leaves, piece_len // LEAF, 0, threads)
    ok = bytearray(np_)
    for i in range(len(layer) // 32):
        ok[i] = layer[32 * i:32 * i + 32] == expected[32 * i:32 * i + 32]
    return bytes(ok)


# Whole torrents. A *unit* is one piece of a file longer than a piece, or one whole smaller
# file; its node is the piece-layer entry, or the file's ``pieces root``. On the device, units of
# many files share one batch (csrc/merkle_plan.h), so a torrent of thousands of small files is
# a handful of copies and launches rather than one round trip per file.

# The device backend of ``verify_files`` / ``hash_files``: the batched entry of the hasher, or
# the per-file loop. Set by the decision rule of docs/PERFORMANCE.md ("Batched across files"):
# both of its conditions held.
GPU_BATCHES_FILES = True


def _check_files(files, piece_len: int) -> List[Tuple[str, int]]:
    check_piece_length(piece_len)
    files = [(str(p), int(n)) for p, n in files]
    if not files:
        raise ValueError("no files")
    if any(n <= 0 for _, n in files):
        raise ValueError("an empty file has no pieces")
    return files


def hash_files(files, piece_len: int, backend: str = "cpu", threads: int = 0) -> bytes:
    """32 bytes per unit of ``files`` (``[(path, length)]``, no empty files), file order then
    piece order: per file its piece layer, or its ``pieces root`` when it is no larger than a
    piece. A missing or short file is an error."""
    files = _check_files(files, piece_len)
    be = choose_backend(backend, sum(n for _, n in files))
    if be == "gpu" and GPU_BATCHES_FILES:
        h = gpu_hasher()
        with _call_lock:
            return h.hash_files(files, int(piece_len))
    out = []
    for p, n in files:
        layer, root = file_tree(p, n, piece_len, backend=be, threads=threads)
        out.append(layer if n > piece_len else root)
    return b"".join(out)


def verify_files(files, piece_len: int, expected, backend: str = "cpu",
                 threads: int = 0) -> bytes:
    """One byte per unit (1 = good) of ``files`` (``[(path, length)]``, no empty files).
    ``expected`` holds one ``bytes`` per file, as ``MetainfoV2.expected`` returns: the piece
    layer of a file longer than a piece, the 32-byte ``pieces root`` otherwise. Units that a
    missing or short file does not cover are 0."""
    files = _check_files(files, piece_len)
    expected = [bytes(e) for e in expected]
    if len(expected) != len(files):
        raise ValueError(f"{len(expected)} expected entries for {len(files)} files")
    for (_, n), e in zip(files, expected):
        want = 32 * (num_pieces(n, piece_len) if n > piece_len else 1)
        if len(e) != want:
            raise ValueError(f"expected is {len(e)} bytes, want {want}")
    be = choose_backend(backend, sum(n for _, n in files), recheck=True)
    if be == "gpu" and GPU_BATCHES_FILES:
        h = gpu_hasher()
        with _call_lock:
            return h.verify_files(files, int(piece_len), b"".join(expected))
    return b"".join(verify_file(p, n, piece_len, e, backend=be, threads=threads)
                    for (p, n), e in zip(files, expected))
