"""BitTorrent v2 metainfo (BEP 52): parse v2-only and hybrid torrents, create v2-only ones.

The v1 parser (``metainfo.parse_torrent``) is untouched: it still refuses a v2-only torrent
(no ``pieces``) and reads a hybrid one as the v1 torrent it also is. This module reads the v2
side - ``file tree``, ``pieces root`` per file and the ``piece layers`` dictionary - and checks
every layer against its root with the CPU tree functions of ``merkle``.

Covered: parse, create, recheck. Not covered: peer-wire hash requests, padding files (BEP 47),
hybrid creation.
"""
from __future__ import annotations

import hashlib
import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

from . import merkle
from .bencode import BencodeError, bencode, decode_torrent
from .metainfo import MetainfoError, _s, _safe, default_piece_length


@dataclass
class FileEntryV2:
    path: List[str]
    length: int
    pieces_root: bytes          # b"" for an empty file
    first_piece: int            # files are piece-aligned in v2: index of the file's first piece
    num_pieces: int


@dataclass
class MetainfoV2:
    info_hash_v2: bytes
    name: str
    piece_length: int
    total_length: int
    files: List[FileEntryV2]
    piece_layers: Dict[bytes, bytes] = field(default_factory=dict)   # keyed by pieces root
    announce: List[List[str]] = field(default_factory=list)
    url_list: List[str] = field(default_factory=list)
    private: bool = False
    comment: str = ""
    raw_info: bytes = b""
    hybrid: bool = False
    multi_file: bool = False

    @property
    def info_hash_v2_short(self) -> bytes:
        """The truncated hash used where 20 bytes are expected (trackers, DHT, handshake)."""
        return self.info_hash_v2[:20]

    @property
    def num_pieces(self) -> int:
        return sum(f.num_pieces for f in self.files)

    def expected(self, f: FileEntryV2) -> bytes:
        """What ``merkle.verify_file`` checks the file against: its piece layer, or its root
        when it is no larger than a piece."""
        return self.piece_layers[f.pieces_root] if f.length > self.piece_length else f.pieces_root

    def local_files(self, root: str) -> List[Tuple[str, int]]:
        """Absolute paths (in file-tree order) and lengths under download dir ``root``: the
        layout rule of v1 (a single file at ``<root>/<name>``, else under ``<root>/<name>/``)."""
        if not self.multi_file:
            return [(os.path.join(root, _safe(self.name)), f.length) for f in self.files]
        base = os.path.join(root, _safe(self.name))
        return [(os.path.join(base, *[_safe(p) for p in f.path]), f.length) for f in self.files]


def _walk(tree: Any, prefix: List[str], out: List[Tuple[List[str], Dict[bytes, Any]]],
          depth: int = 0) -> None:
    """Files of a ``file tree`` in tree order. A node is a directory (a dictionary of named
    nodes) or a file, ``{"": {"length": ..., "pieces root": ...}}``."""
    if not isinstance(tree, dict) or not tree:
        raise MetainfoError("file tree node is neither a directory nor a file")
    if depth > 64:
        raise MetainfoError("file tree nested too deep")
    for key, node in tree.items():
        if key == b"":
            raise MetainfoError("file tree: a file entry beside directory entries")
        if not isinstance(node, dict) or not node:
            raise MetainfoError("file tree node is neither a directory nor a file")
        path = prefix + [_s(key)]
        if b"" in node:
            if len(node) != 1 or not isinstance(node[b""], dict):
                raise MetainfoError("file tree node is neither a directory nor a file")
            out.append((path, node[b""]))
        else:
            _walk(node, path, out, depth + 1)


def _parse_checked(top: Dict[bytes, Any], raw: bytes) -> MetainfoV2:
    info = top[b"info"]
    if not isinstance(info, dict):
        raise MetainfoError("info is not a dictionary")
    if info.get(b"meta version") != 2:
        raise MetainfoError(f"meta version {info.get(b'meta version')!r} is not 2")
    plen = info.get(b"piece length")
    try:
        level = merkle.check_piece_length(plen)
    except ValueError as e:
        raise MetainfoError(f"bad piece length: {e}") from e
    if b"file tree" not in info:
        raise MetainfoError("info dict missing field: 'file tree'")
    found: List[Tuple[List[str], Dict[bytes, Any]]] = []
    _walk(info[b"file tree"], [], found)
    layers_in = top.get(b"piece layers", {})
    if not isinstance(layers_in, dict):
        raise MetainfoError("piece layers is not a dictionary")
    name = _s(info.get(b"name.utf-8", info.get(b"name")), "torrent")
    files: List[FileEntryV2] = []
    layers: Dict[bytes, bytes] = {}
    piece = 0
    for path, leaf in found:
        ln = leaf.get(b"length")
        if not isinstance(ln, int) or ln < 0:
            raise MetainfoError("file entry without a valid length")
        root = leaf.get(b"pieces root", b"")
        if ln == 0:
            files.append(FileEntryV2(path, 0, b"", piece, 0))
            continue
        if not isinstance(root, bytes) or len(root) != 32:
            raise MetainfoError("pieces root is not 32 bytes")
        n = merkle.num_pieces(ln, plen)
        if ln > plen:
            layer = layers_in.get(root)
            if not isinstance(layer, bytes):
                raise MetainfoError(f"piece layer of {'/'.join(path)} is missing")
            if len(layer) != 32 * n:
                raise MetainfoError(f"piece layer of {'/'.join(path)} is {len(layer)} bytes, "
                                    f"want {32 * n}")
            if merkle.layer_root(layer, level) != root:
                raise MetainfoError(f"piece layer of {'/'.join(path)} does not hash to its root")
            layers[root] = layer
        files.append(FileEntryV2(path, ln, root, piece, n))
        piece += n
    hybrid = b"pieces" in info and (b"files" in info or b"length" in info)
    if hybrid:
        multi = b"files" in info
    else:
        multi = not (len(files) == 1 and files[0].path == [name])
    return MetainfoV2(hashlib.sha256(raw).digest(), name, plen, sum(f.length for f in files),
                      files, layers, private=bool(info.get(b"private", 0)), raw_info=raw,
                      hybrid=hybrid, multi_file=multi)


def parse_torrent_v2(data: bytes) -> MetainfoV2:
    """The v2 side of a v2-only or hybrid torrent. Anything malformed is a MetainfoError,
    never another exception type."""
    try:
        top, info_bytes = decode_torrent(data)
    except BencodeError as e:
        raise MetainfoError(f"not a torrent: {e}") from e
    if not isinstance(top, dict) or b"info" not in top:
        raise MetainfoError("not a torrent: no info dictionary")
    try:
        m = _parse_checked(top, info_bytes)
    except MetainfoError:
        raise
    except (KeyError, TypeError, ValueError, AttributeError, OverflowError, RecursionError) as e:
        raise MetainfoError(f"malformed v2 torrent: {type(e).__name__}: {e}") from e
    tiers: List[List[str]] = []
    al = top.get(b"announce-list")
    if isinstance(al, list):            # a malformed list is ignored, as in v1
        for tier in al:
            t = [_s(u) for u in tier if u] if isinstance(tier, list) else []
            if t:
                tiers.append(t)
    if b"announce" in top and not tiers:
        tiers.append([_s(top[b"announce"])])
    m.announce = tiers
    ul = top.get(b"url-list")
    if isinstance(ul, (bytes, str)):
        m.url_list = [_s(ul)] if ul else []
    elif isinstance(ul, list):
        m.url_list = [_s(u) for u in ul if u]
    m.comment = _s(top.get(b"comment"))
    return m


def make_torrent_v2(path: str, piece_length: int = 0, trackers: Sequence[str] = (),
                    url_list: Sequence[str] = (), name: Optional[str] = None,
                    private: bool = False, threads: int = 0, comment: str = "",
                    backend: str = "cpu") -> bytes:
    """Create a v2-only .torrent for a file or a directory. Dictionary keys are sorted by raw
    bytes (``bencode``), so the file tree comes out in the order BEP 52 asks for."""
    path = os.path.abspath(path)
    if os.path.isdir(path):
        rels: List[Tuple[List[str], str, int]] = []
        for dp, dns, fns in os.walk(path):
            dns.sort()
            for fn in sorted(fns):
                ap = os.path.join(dp, fn)
                rels.append((os.path.relpath(ap, path).split(os.sep), ap, os.path.getsize(ap)))
    else:
        rels = [([name or os.path.basename(path)], path, os.path.getsize(path))]
    total = sum(r[2] for r in rels)
    plen = piece_length or default_piece_length(total)
    merkle.check_piece_length(plen)
    tree: Dict[bytes, Any] = {}
    layers: Dict[bytes, bytes] = {}
    for rel, ap, n in rels:
        node = tree
        for part in rel:
            node = node.setdefault(os.fsencode(part), {})
        leaf: Dict[str, Any] = {"length": n}
        if n:
            layer, root = merkle.file_tree(ap, n, plen, backend=backend, threads=threads)
            leaf["pieces root"] = root
            if layer:
                layers[root] = layer
        node[b""] = leaf
    info: Dict[str, Any] = {"name": name or os.path.basename(path), "file tree": tree,
                            "meta version": 2, "piece length": plen}
    if private:
        info["private"] = 1
    top: Dict[str, Any] = {"info": info, "piece layers": layers, "created by": "downloader-amd"}
    if trackers:
        top["announce"] = trackers[0]
        top["announce-list"] = [[t] for t in trackers]
    if url_list:
        top["url-list"] = list(url_list)
    if comment:
        top["comment"] = comment
    return bencode(top)
