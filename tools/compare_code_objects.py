#!/usr/bin/env python3
"""Compare the kernels of two sets of gfx950 code objects symbol by symbol.

    python tools/compare_code_objects.py --before a.co [b.co ...] --after c.co [d.co ...]

A code object is what `hipcc --offload-arch=gfx950 <the project's flags> --cuda-device-only
--no-gpu-bundle-output -c unit.hip -o unit.co` writes.  For a change that only moves kernels between
translation units, every function of the `before` set must turn up in exactly one object of the `after`
set with the same size and the same bytes, and its kernel descriptor (`<name>.kd`, 64 bytes) must be equal
once the code-entry offset (bytes 16-23, the distance from the descriptor to the code) is masked.

Prints the symbols that are missing from `after`, new in `after`, defined more than once within a set, and
differing; exit status 1 when anything but `missing` is non-empty (`--allow-missing N` also bounds those).
Nothing is disassembled.
"""
from __future__ import annotations

import argparse
import struct
import sys

STT_OBJECT, STT_FUNC = 1, 2
KD_SIZE, KD_ENTRY = 64, slice(16, 24)


def symbols(path: str) -> dict[str, bytes]:
    """{name: bytes} of the defined functions and kernel descriptors of one ELF64 little-endian object."""
    blob = open(path, "rb").read()
    if blob[:6] != b"\x7fELF\x02\x01":
        raise SystemExit(f"{path}: not a little-endian ELF64 file")
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    out: dict[str, bytes] = {}
    for sec in secs:
        if sec[1] != 2:   # SHT_SYMTAB
            continue
        _, _, _, _, off, size, link, _, _, entsize = sec
        stroff = secs[link][4]
        for i in range(size // entsize):
            name_i, info, _, shndx, value, sz = struct.unpack_from("<IBBHQQ", blob, off + i * entsize)
            kind = info & 0xF
            if kind not in (STT_FUNC, STT_OBJECT) or shndx == 0 or shndx >= 0xFF00 or sz == 0:
                continue
            name = blob[stroff + name_i:blob.index(b"\0", stroff + name_i)].decode()
            if kind == STT_OBJECT and not name.endswith(".kd"):
                continue
            s = secs[shndx]
            if s[1] == 8:   # SHT_NOBITS
                continue
            start = s[4] + value - s[3]
            data = blob[start:start + sz]
            if name.endswith(".kd") and len(data) == KD_SIZE:
                data = data[:KD_ENTRY.start] + bytes(8) + data[KD_ENTRY.stop:]
            out[name] = data
    return out


def collect(paths: list[str]) -> tuple[dict[str, tuple[str, bytes]], list[str]]:
    merged: dict[str, tuple[str, bytes]] = {}
    dup = []
    for p in paths:
        for name, data in symbols(p).items():
            if name in merged:
                dup.append(f"{name}  ({merged[name][0]} and {p})")
            merged[name] = (p, data)
    return merged, dup


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    ap.add_argument("--allow-missing", type=int, default=None, help="fail when more symbols than this are missing")
    a = ap.parse_args()
    before, dup_b = collect(a.before)
    after, dup_a = collect(a.after)
    missing = sorted(n for n in before if n not in after)
    new = sorted(n for n in after if n not in before)
    differing = []
    for n in sorted(before):
        if n in after and before[n][1] != after[n][1]:
            differing.append(f"{n}  ({len(before[n][1])} -> {len(after[n][1])} bytes, now in {after[n][0]})")
    nk = sum(1 for n in before if n.endswith(".kd"))
    print(f"before: {len(before)} symbols ({nk} kernel descriptors) in {len(a.before)} object(s)")
    print(f"after:  {len(after)} symbols ({sum(1 for n in after if n.endswith('.kd'))} kernel descriptors) "
          f"in {len(a.after)} object(s)")
    for p in a.after:
        print(f"  {p}: {sum(1 for n, (q, _) in after.items() if q == p and n.endswith('.kd'))} kernels")
    for title, rows in (("missing from after", missing), ("new in after", new),
                        ("defined twice", dup_b + dup_a), ("differing", differing)):
        print(f"{title}: {len(rows)}")
        for r in rows:
            print(f"  {r}")
    print(f"identical: {len(before) - len(missing) - len(differing)}")
    bad = bool(new or dup_b or dup_a or differing)
    if a.allow_missing is not None and len(missing) > a.allow_missing:
        bad = True
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
