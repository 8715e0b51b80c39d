"""What the hashing entry points accept as a buffer: C-contiguous bytes, nothing else.

``view()`` in ``csrc/module.cpp`` and the buffer entries of ``_gpuhash`` hash
``size * itemsize`` bytes from the buffer's pointer. For a stepped, reversed or column slice
those are not the view's bytes - the digest came out wrong with no error, and a reversed view
would have been read from before its first byte - so every such view is a ``ValueError``, on
the host and (before any HIP call) on the device. What is contiguous is hashed as its
``tobytes()``, whatever its item size or rank.
"""
from __future__ import annotations

import hashlib
import random

import numpy as np
import pytest

SEED = 901
BLOB = random.Random(SEED).randbytes(1024)


def base():
    return np.frombuffer(BLOB, dtype=np.uint8)


REFUSED = {
    "step2": lambda: base()[::2],
    "reversed": lambda: base()[::-1],
    "column-slice-2d": lambda: base().reshape(32, 32)[:, :16],
    "uint32-step2": lambda: base().view(np.uint32)[::2],
    "memoryview-step2": lambda: memoryview(BLOB)[::2],
    "rows-step2-2d": lambda: base().reshape(32, 32)[::2],
}
ACCEPTED = {
    "bytearray": lambda: bytearray(BLOB),
    "memoryview-slice": lambda: memoryview(BLOB)[100:900],
    "uint32": lambda: base().view(np.uint32),
    "2d": lambda: base().reshape(32, 32),
    "2d-row-slice": lambda: base().reshape(32, 32)[4:20],
    "column-slice-of-one-row": lambda: base().reshape(1, 1024)[:, 10:522],
}
EMPTY = {
    "empty-bytes": lambda: b"",
    "empty-2d": lambda: np.empty((0, 4), dtype=np.uint32),
    "empty-of-a-stepped-view": lambda: base()[::2][:0],
}


def ids(table):
    return [pytest.param(table[k], id=f"{k}-seed{SEED}") for k in table]


def raw(buf):
    return memoryview(buf).tobytes()


def ref(data, piece):
    return b"".join(hashlib.sha1(data[i:i + piece]).digest() for i in range(0, len(data), piece))


def crc32c_ref(data, crc=0):
    """Bitwise CRC32C (Castagnoli, reflected polynomial 0x82F63B78)."""
    crc ^= 0xFFFFFFFF
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ (0x82F63B78 if crc & 1 else 0)
    return crc ^ 0xFFFFFFFF


def test_the_cases_are_what_they_claim():
    assert crc32c_ref(b"123456789") == 0xE3069283
    for make in REFUSED.values():
        m = memoryview(make())
        assert not m.c_contiguous and m.nbytes > 0
    for make in list(ACCEPTED.values()) + list(EMPTY.values()):
        assert memoryview(make()).c_contiguous
    for make in EMPTY.values():
        assert memoryview(make()).nbytes == 0
    assert {memoryview(make()).itemsize for make in ACCEPTED.values()} == {1, 4}
    assert {memoryview(make()).ndim for make in ACCEPTED.values()} == {1, 2}


# ------------------------------------------------------------ the host module (no device)
def host_entries():
    from downloader_amd.ops import native
    n = native()

    def hasher(buf):
        h = n.Hasher("sha1")
        h.update(buf)
        return h.digest()

    return {
        "digest": (lambda buf: n.digest("sha1", buf), lambda d: hashlib.sha1(d).digest()),
        "digest-sha256": (lambda buf: n.digest("sha256", buf),
                          lambda d: hashlib.sha256(d).digest()),
        "crc32c": (lambda buf: n.crc32c(buf, 7), lambda d: crc32c_ref(d, 7)),
        "hash_pieces": (lambda buf: n.hash_pieces("sha1", buf, 100, 2), lambda d: ref(d, 100)),
        "Hasher.update": (hasher, lambda d: hashlib.sha1(d).digest()),
    }


HOST = ["digest", "digest-sha256", "crc32c", "hash_pieces", "Hasher.update"]


@pytest.mark.parametrize("entry", HOST)
@pytest.mark.parametrize("make", ids(REFUSED))
def test_host_entries_refuse_what_is_not_contiguous(entry, make):
    call, _ = host_entries()[entry]
    with pytest.raises(ValueError):
        call(make())


@pytest.mark.parametrize("entry", HOST)
@pytest.mark.parametrize("make", ids(ACCEPTED) + ids(EMPTY))
def test_host_entries_hash_contiguous_buffers_as_their_bytes(entry, make):
    call, want = host_entries()[entry]
    buf = make()
    assert call(buf) == want(raw(buf))


def test_front_end_refuses_a_stepped_view():
    from downloader_amd.ops import hashing
    for make in REFUSED.values():
        with pytest.raises(ValueError):
            hashing.sha1(make())
        with pytest.raises(ValueError):
            hashing.hash_pieces(make(), 100)
    assert hashing.sha1(base().view(np.uint32)) == hashlib.sha1(BLOB).digest()


# --------------------------------------------------------------------------- on the device
@pytest.fixture(scope="module")
def gv():
    from downloader_amd.ops import gpu_available, gpuhash
    if not gpu_available():
        pytest.fail("HIP device not visible: the GPU test tier must run on a MI355X")
    assert "gfx950" in gpuhash().arch()
    return gpuhash().GpuVerifier(0, 64 * 1024, 2)


@pytest.fixture(scope="module")
def part_hasher(gv):
    from downloader_amd.ops import gpuhash
    return gpuhash().PartHasher(0, 4 << 20, 2, 1, 64)


def lanes_of(n):
    return [0, 16], [n, min(100, n - 16)]


def lanes_ref(data):
    offs, lens = lanes_of(len(data))
    return b"".join(hashlib.sha1(data[o:o + n]).digest() for o, n in zip(offs, lens))


def device_entries(gv, part_hasher):
    return {
        "hash_buffer": (lambda buf: gv.hash_buffer(buf, 100), lambda d: ref(d, 100)),
        "hash_lanes": (lambda buf: gv.hash_lanes(buf, *lanes_of(memoryview(buf).nbytes), "split"),
                       lanes_ref),
        "hash_pieces_variant": (lambda buf: gv.hash_pieces_variant(buf, 64, "default"),
                                lambda d: ref(d, 64)),
        "PartHasher.hash": (lambda buf: part_hasher.hash(buf, 256), lambda d: ref(d, 256)),
    }


DEVICE = ["hash_buffer", "hash_lanes", "hash_pieces_variant", "PartHasher.hash"]


@pytest.mark.gpu
@pytest.mark.parametrize("entry", DEVICE)
def test_device_entries_refuse_what_is_not_contiguous(gv, part_hasher, entry):
    """Refused before any HIP call and before PartHasher::reg: nothing of the view is read."""
    call, want = device_entries(gv, part_hasher)[entry]
    before = part_hasher.stats()
    for name, make in REFUSED.items():
        with pytest.raises(ValueError):
            call(make())
    after = part_hasher.stats()
    assert (after["registered"], after["submitted"]) == (before["registered"], before["submitted"])
    assert call(BLOB) == want(BLOB)               # and the entry still serves


@pytest.mark.gpu
@pytest.mark.parametrize("entry", DEVICE)
def test_device_entries_hash_contiguous_buffers_as_their_bytes(gv, part_hasher, entry):
    call, want = device_entries(gv, part_hasher)[entry]
    for name, make in ACCEPTED.items():
        buf = make()
        assert call(buf) == want(raw(buf)), (entry, name)


@pytest.mark.gpu
def test_hash_buffer_of_an_empty_buffer(gv):
    """The one device entry that allows a zero-length buffer: no pieces, no digests."""
    for name, make in EMPTY.items():
        assert gv.hash_buffer(make(), 100) == b"", name
