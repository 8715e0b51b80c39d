"""BitTorrent v2 (BEP 52) on the CPU tier: tree rules, v2 metainfo, recheck and the CLI.

The reference everywhere is hashlib through an independent recursive tree written here:
``root(nodes) = sha256(root(left half) + root(right half))``. Equality is bit-exact.
"""
from __future__ import annotations

import hashlib
import json
import os

import pytest

from downloader_amd.torrent.bencode import bdecode, bencode
from downloader_amd.torrent.metainfo import MetainfoError, make_torrent, parse_torrent

LEAF = 16384
PAD1 = bytes.fromhex("f5a5fd42d16a20302798ef6ed309979b43003d2320d9f0e8ea9831a92759fb4b")


def sha256(b: bytes) -> bytes:
    return hashlib.sha256(b).digest()


def ref_root(nodes):
    """Root of a power-of-two list of 32-byte nodes."""
    if len(nodes) == 1:
        return nodes[0]
    h = len(nodes) // 2
    return sha256(ref_root(nodes[:h]) + ref_root(nodes[h:]))


def pow2(n: int) -> int:
    p = 1
    while p < n:
        p *= 2
    return p


def ref_pad(level: int) -> bytes:
    return ref_root([bytes(32)] * (1 << level))


def ref_tree(data: bytes, piece_len: int):
    """(piece_layer, root) by the rules of BEP 52, straight from the bytes."""
    leaves = [sha256(data[i:i + LEAF]) for i in range(0, len(data), LEAF)]
    if len(data) <= piece_len:
        return b"", ref_root(leaves + [bytes(32)] * (pow2(len(leaves)) - len(leaves)))
    per = piece_len // LEAF
    layer = []
    for i in range(0, len(leaves), per):
        grp = leaves[i:i + per]
        layer.append(ref_root(grp + [bytes(32)] * (per - len(grp))))
    level = per.bit_length() - 1
    root = ref_root(layer + [ref_pad(level)] * (pow2(len(layer)) - len(layer)))
    return b"".join(layer), root


def blob(n: int, seed: int = 1) -> bytes:
    out = bytearray()
    h = hashlib.sha256(b"seed%d" % seed).digest()
    while len(out) < n:
        h = hashlib.sha256(h).digest()
        out += h * 64
    return bytes(out[:n])


def test_pad_hash_constant():
    from downloader_amd.torrent import merkle
    assert merkle.pad_hash(0) == bytes(32)
    assert merkle.pad_hash(1) == PAD1 == sha256(bytes(64))
    assert merkle.pad_hash(5) == ref_pad(5)


@pytest.mark.parametrize("piece_len", [16384, 32768, 65536])
@pytest.mark.parametrize("length", [1, 16384, 16385, 3 * 16384, 5 * 16384 + 7])
def test_file_tree_cpu_matches_recursive_reference(tmp_path, length, piece_len):
    from downloader_amd.torrent import merkle
    data = blob(length, length)
    p = tmp_path / "f.bin"
    p.write_bytes(data)
    layer, root = merkle.file_tree(str(p), length, piece_len, backend="cpu")
    want_layer, want_root = ref_tree(data, piece_len)
    assert layer == want_layer
    assert root == want_root
    assert (layer == b"") == (length <= piece_len)
    assert merkle.leaf_hashes(data) == b"".join(
        sha256(data[i:i + LEAF]) for i in range(0, length, LEAF))


def test_file_tree_edge_arguments(tmp_path):
    from downloader_amd.torrent import merkle
    p = tmp_path / "e.bin"
    p.write_bytes(b"")
    assert merkle.file_tree(str(p), 0, 16384) == (b"", b"")
    for bad in (24576, 8192, 0, 512 << 20):
        with pytest.raises(ValueError):
            merkle.file_tree(str(p), 0, bad)
    with pytest.raises(ValueError):
        merkle.file_tree(str(p), 0, 16384, backend="tpu")


LENGTHS = {"a/empty.bin": 0, "a/one.bin": 1, "b.bin": 16384, "c/d/mid.bin": 40000,
           "z.bin": 300000}


def make_dir(tmp_path):
    root = tmp_path / "pack"
    datas = {}
    for i, (rel, n) in enumerate(LENGTHS.items()):
        fp = root / rel
        fp.parent.mkdir(parents=True, exist_ok=True)
        datas[rel] = blob(n, 100 + i)
        fp.write_bytes(datas[rel])
    return root, datas


def test_make_then_parse_round_trip(tmp_path):
    from downloader_amd.torrent.metainfo_v2 import make_torrent_v2, parse_torrent_v2
    root, datas = make_dir(tmp_path)
    plen = 32768
    raw = make_torrent_v2(str(root), plen, trackers=["http://t.example/announce"],
                          url_list=["http://w.example/"], comment="hello", private=True)
    m = parse_torrent_v2(raw)
    assert m.info_hash_v2 == sha256(m.raw_info) and m.info_hash_v2_short == m.info_hash_v2[:20]
    assert bencode(bdecode(raw)[b"info"]) == m.raw_info            # keys sorted by raw bytes
    assert m.name == "pack" and m.piece_length == plen and not m.hybrid and m.private
    assert m.announce == [["http://t.example/announce"]] and m.url_list == ["http://w.example/"]
    assert m.comment == "hello"
    assert ["/".join(f.path) for f in m.files] == sorted(LENGTHS)   # file-tree order
    assert m.total_length == sum(LENGTHS.values())
    first = 0
    for f in m.files:
        rel = "/".join(f.path)
        n = LENGTHS[rel]
        assert f.length == n and f.first_piece == first
        assert f.num_pieces == (n + plen - 1) // plen
        first += f.num_pieces
        if n == 0:
            assert f.pieces_root == b"" and f.num_pieces == 0
            continue
        want_layer, want_root = ref_tree(datas[rel], plen)
        assert f.pieces_root == want_root
        if n <= plen:
            assert f.pieces_root not in m.piece_layers
        else:
            assert m.piece_layers[f.pieces_root] == want_layer
    assert first == m.num_pieces == 0 + 1 + 1 + 2 + 10
    assert set(m.piece_layers) == {f.pieces_root for f in m.files if f.length > plen}
    info = bdecode(m.raw_info)
    assert b"pieces root" not in info[b"file tree"][b"a"][b"empty.bin"][b""]
    assert m.local_files("/dl") == [(os.path.join("/dl", "pack", *rel.split("/")), LENGTHS[rel])
                                    for rel in sorted(LENGTHS)]
    # a single file lands at <root>/<name>, as in v1
    one = parse_torrent_v2(make_torrent_v2(str(root / "z.bin"), plen))
    assert one.local_files("/dl") == [("/dl/z.bin", 300000)]
    assert one.files[0].pieces_root == ref_tree(datas["z.bin"], plen)[1]


def v2_parts(data: bytes, plen: int, fname: bytes = b"f.bin"):
    """(info dict, piece layers dict) of a one-file v2 torrent, assembled by hand."""
    layer, root = ref_tree(data, plen)
    info = {b"name": fname, b"piece length": plen, b"meta version": 2,
            b"file tree": {fname: {b"": {b"length": len(data), b"pieces root": root}}}}
    return info, ({root: layer} if layer else {})


def test_hybrid_torrent_is_read_by_both_parsers(tmp_path):
    from downloader_amd.torrent.metainfo_v2 import parse_torrent_v2
    data = blob(100000, 7)
    plen = 32768
    p = tmp_path / "f.bin"
    p.write_bytes(data)
    v1 = parse_torrent(make_torrent(str(p), plen))
    info, layers = v2_parts(data, plen)
    info[b"length"] = len(data)
    info[b"pieces"] = v1.pieces
    raw = bencode({b"info": info, b"piece layers": layers, b"announce": b"http://t/a"})
    m1 = parse_torrent(raw)
    assert (m1.name, m1.piece_length, m1.pieces, m1.total_length, m1.multi_file) == \
        ("f.bin", plen, v1.pieces, len(data), False)
    assert m1.pieces == b"".join(hashlib.sha1(data[i:i + plen]).digest()
                                 for i in range(0, len(data), plen))
    assert m1.info_hash == hashlib.sha1(bencode(info)).digest()
    assert [(f.path, f.length, f.offset) for f in m1.files] == [(["f.bin"], len(data), 0)]
    assert m1.announce == [["http://t/a"]]
    m2 = parse_torrent_v2(raw)
    assert m2.hybrid and m2.info_hash_v2 == sha256(bencode(info))
    assert m2.files[0].pieces_root == ref_tree(data, plen)[1]
    assert m2.local_files("/dl") == m1.local_files("/dl")


def test_v1_parser_still_refuses_a_v2_only_torrent():
    from downloader_amd.torrent.metainfo_v2 import parse_torrent_v2
    info, layers = v2_parts(blob(100000, 8), 32768)
    raw = bencode({b"info": info, b"piece layers": layers})
    assert parse_torrent_v2(raw).num_pieces == 4
    with pytest.raises(MetainfoError):
        parse_torrent(raw)


def _mutations():
    data = blob(100000, 9)          # 4 pieces of 32 KiB
    plen = 32768
    _, root = ref_tree(data, plen)

    def case(fn):
        info, layers = v2_parts(data, plen)
        top = {b"info": info, b"piece layers": layers}
        fn(top, info, layers)
        return bencode(top)

    def leaf(info):
        return info[b"file tree"][b"f.bin"][b""]

    def wrong_layer(top, info, layers):
        layers[root] = layers[root][:32] + bytes(32) + layers[root][64:]

    return {
        "meta version 1": case(lambda t, i, l: i.__setitem__(b"meta version", 1)),
        "meta version missing": case(lambda t, i, l: i.pop(b"meta version")),
        "piece length not a power of two": case(lambda t, i, l: i.__setitem__(b"piece length", 24576)),
        "piece length below 16 KiB": case(lambda t, i, l: i.__setitem__(b"piece length", 8192)),
        "piece length not an integer": case(lambda t, i, l: i.__setitem__(b"piece length", b"x")),
        "piece length above the maximum": case(lambda t, i, l: i.__setitem__(b"piece length", 1 << 30)),
        "node is a string": case(lambda t, i, l: i[b"file tree"].__setitem__(b"g.bin", b"oops")),
        "node is an empty directory": case(lambda t, i, l: i[b"file tree"].__setitem__(b"g", {})),
        "file leaf with siblings": case(
            lambda t, i, l: i[b"file tree"][b"f.bin"].__setitem__(b"x", {b"": {b"length": 0}})),
        "file tree is a list": case(lambda t, i, l: i.__setitem__(b"file tree", [1])),
        "root is 20 bytes": case(lambda t, i, l: leaf(i).__setitem__(b"pieces root", root[:20])),
        "root missing": case(lambda t, i, l: leaf(i).pop(b"pieces root")),
        "layer missing": case(lambda t, i, l: l.clear()),
        "piece layers missing": case(lambda t, i, l: t.pop(b"piece layers")),
        "layer too short": case(lambda t, i, l: l.__setitem__(root, l[root][:-32])),
        "layer too long": case(lambda t, i, l: l.__setitem__(root, l[root] + bytes(32))),
        "layer does not hash to the root": case(wrong_layer),
        "negative length": case(lambda t, i, l: leaf(i).__setitem__(b"length", -1)),
    }


MUTATIONS = _mutations()


@pytest.mark.parametrize("what", sorted(MUTATIONS))
def test_malformed_v2_torrent_is_a_metainfo_error(what):
    from downloader_amd.torrent.metainfo_v2 import parse_torrent_v2
    with pytest.raises(MetainfoError):
        parse_torrent_v2(MUTATIONS[what])


def test_well_formed_hand_made_torrent_parses():
    """The base of every mutation above is accepted: the cases fail for their own reason."""
    from downloader_amd.torrent.metainfo_v2 import parse_torrent_v2
    info, layers = v2_parts(blob(100000, 9), 32768)
    m = parse_torrent_v2(bencode({b"info": info, b"piece layers": layers}))
    assert m.files[0].num_pieces == 4 and not m.hybrid
    for junk in (b"", b"i1e", b"de", b"d4:infoi1ee"):
        with pytest.raises(MetainfoError):
            parse_torrent_v2(junk)


def flip(path, offset: int) -> None:
    with open(path, "r+b") as f:
        f.seek(offset)
        b = f.read(1)
        f.seek(offset)
        f.write(bytes([b[0] ^ 0x01]))


def test_verify_file_cpu(tmp_path):
    from downloader_amd.torrent import merkle
    plen = 32768
    n = 5 * plen + 1000                     # six pieces, a short last one
    data = blob(n, 11)
    p = tmp_path / "v.bin"
    p.write_bytes(data)
    layer, _root = ref_tree(data, plen)
    assert merkle.verify_file(str(p), n, plen, layer) == b"\x01" * 6
    flip(p, 2 * plen + 777)
    assert merkle.verify_file(str(p), n, plen, layer) == b"\x01\x01\x00\x01\x01\x01"
    flip(p, 2 * plen + 777)
    flip(p, n - 1)                          # in the short last piece
    assert merkle.verify_file(str(p), n, plen, layer) == b"\x01\x01\x01\x01\x01\x00"
    flip(p, n - 1)
    with open(p, "r+b") as f:               # truncated inside piece 3
        f.truncate(3 * plen + 5)
    assert merkle.verify_file(str(p), n, plen, layer) == b"\x01\x01\x01\x00\x00\x00"
    os.unlink(p)
    assert merkle.verify_file(str(p), n, plen, layer) == bytes(6)
    with pytest.raises(ValueError):
        merkle.verify_file(str(p), n, plen, layer[:-32])
    # a file no larger than a piece is checked against its root: exactly one byte
    small = blob(20000, 12)
    q = tmp_path / "s.bin"
    q.write_bytes(small)
    root = ref_tree(small, plen)[1]
    assert merkle.verify_file(str(q), 20000, plen, root) == b"\x01"
    flip(q, 19999)
    assert merkle.verify_file(str(q), 20000, plen, root) == b"\x00"
    flip(q, 19999)
    with open(q, "r+b") as f:
        f.truncate(16384)
    assert merkle.verify_file(str(q), 20000, plen, root) == b"\x00"


def test_cli_make_and_verify_v2(tmp_path, capsys):
    from downloader_amd.__main__ import main
    root, _ = make_dir(tmp_path)
    tor = tmp_path / "pack.torrent"
    assert main(["make-torrent", str(root), "-o", str(tor), "--piece-length", "32768",
                 "--meta-version", "2"]) == 0
    made = json.loads(capsys.readouterr().out)
    assert made["meta_version"] == 2 and made["pieces"] == 14 and made["piece_length"] == 32768
    assert made["bytes"] == sum(LENGTHS.values())
    assert made["info_hash"] == sha256(
        bencode(bdecode(tor.read_bytes())[b"info"])).hex()
    assert main(["verify", str(tor), str(tmp_path), "--backend", "cpu"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["meta_version"] == 2 and out["pieces"] == out["good"] == 14
    assert set(out) == {"pieces", "good", "seconds", "GBps", "backend", "meta_version"}
    assert out["backend"] == "cpu"
    flip(root / "z.bin", 70000)
    assert main(["verify", str(tor), str(tmp_path), "--backend", "cpu"]) == 1
    out = json.loads(capsys.readouterr().out)
    assert out["pieces"] == 14 and out["good"] == 13


def test_cli_verify_merkle_flag_on_a_hybrid(tmp_path, capsys):
    from downloader_amd.__main__ import main
    data = blob(100000, 7)
    plen = 32768
    (tmp_path / "f.bin").write_bytes(data)
    v1 = parse_torrent(make_torrent(str(tmp_path / "f.bin"), plen))
    info, layers = v2_parts(data, plen)
    info[b"length"] = len(data)
    info[b"pieces"] = v1.pieces
    tor = tmp_path / "h.torrent"
    tor.write_bytes(bencode({b"info": info, b"piece layers": layers}))
    assert main(["verify", str(tor), str(tmp_path), "--backend", "cpu"]) == 0
    assert "meta_version" not in json.loads(capsys.readouterr().out)      # the v1 recheck
    assert main(["verify", str(tor), str(tmp_path), "--backend", "cpu", "--merkle"]) == 0
    out = json.loads(capsys.readouterr().out)
    assert out["meta_version"] == 2 and out["pieces"] == out["good"] == 4


def test_cli_make_torrent_default_is_byte_identical_to_v1(tmp_path, capsys):
    from downloader_amd.__main__ import main
    root, _ = make_dir(tmp_path)
    for extra in ([], ["--meta-version", "1"]):
        tor = tmp_path / "v1.torrent"
        assert main(["make-torrent", str(root), "-o", str(tor), "--piece-length", "32768",
                     "--tracker", "http://t.example/a", *extra]) == 0
        assert "meta_version" not in json.loads(capsys.readouterr().out)
        assert tor.read_bytes() == make_torrent(str(root), 32768, ["http://t.example/a"], [])
