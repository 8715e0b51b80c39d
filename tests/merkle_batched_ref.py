"""What the batched-merkle tests share: an independent recursive hashlib tree (the reference
everywhere; equality is bit-exact), seeded file contents and the unit rules of BEP 52."""
from __future__ import annotations

import hashlib
import random

LEAF = 16384
ZERO = bytes(32)


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


def ref_nodes(data: bytes, piece_len: int):
    """The unit nodes of one file: its piece layer, or [its pieces root] when it is no larger
    than a piece."""
    leaves = [sha256(data[i:i + LEAF]) for i in range(0, len(data), LEAF)]
    if len(data) <= piece_len:
        return [ref_root(leaves + [ZERO] * (pow2(len(leaves)) - len(leaves)))]
    per = piece_len // LEAF
    return [ref_root(leaves[i:i + per] + [ZERO] * (per - len(leaves[i:i + per])))
            for i in range(0, len(leaves), per)]


def blob(n: int, seed) -> bytes:
    return random.Random(f"batched-{seed}").randbytes(n)


def mixed_lengths(piece_len: int):
    """The issue's file lengths: every width from 1 up to the piece's, short last leaves, a
    file of exactly one piece, one byte more, and two pieces."""
    return [1, 16384, 16385, 3 * 16384 + 55, 4 * 16384, 5 * 16384 + 7, 9 * 16384, piece_len,
            piece_len + 1, 2 * piece_len]


def ordered(lengths, order: str):
    if order == "ascending":
        return sorted(lengths)
    if order == "descending":
        return sorted(lengths, reverse=True)
    out = list(lengths)
    random.Random(f"order-{len(lengths)}").shuffle(out)
    return out


def units_of(length: int, piece_len: int) -> int:
    return (length + piece_len - 1) // piece_len if length > piece_len else 1


def write_files(root, datas):
    """datas -> [(path, length)], files f0000.bin ... in `root`."""
    root.mkdir(parents=True, exist_ok=True)
    files = []
    for i, d in enumerate(datas):
        p = root / f"f{i:04d}.bin"
        p.write_bytes(d)
        files.append((str(p), len(d)))
    return files


def flip(path, offset: int, bit: int = 0) -> None:
    with open(path, "r+b") as f:
        f.seek(offset)
        b = f.read(1)
        f.seek(offset)
        f.write(bytes([b[0] ^ (1 << bit)]))
