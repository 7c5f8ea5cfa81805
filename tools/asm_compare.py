#!/usr/bin/env python3
"""Compare the gfx950 code generated from two checkouts, kernel by kernel.

Usage: ``python tools/asm_compare.py PARENT_CHECKOUT CHANGE_CHECKOUT [--jobs N] [--keep DIR]``.

Every ``pmarlo_amd/csrc/*.hip`` of both checkouts is compiled with the flags of
``build.py`` plus ``--cuda-device-only -S``.  For each kernel the script compares
the resource metadata (VGPRs, SGPRs, AGPRs, scratch, LDS) and the histogram of
instruction mnemonics, prints one table row per kernel that differs and a
summary line per file, and exits non-zero if anything differs.  No GPU needed.
"""

from __future__ import annotations

import argparse
import collections
import importlib.util
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

META_KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")
# a difference in one of these is a defect, not a scheduling artefact
STRICT = re.compile(r"^(v_\w*_f64\w*|v_mfma\w*|s_waitcnt\w*|s_barrier)$")


def _flags(checkout: Path) -> list[str]:
    spec = importlib.util.spec_from_file_location("_b", checkout / "pmarlo_amd/csrc/build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [f for f in mod.FLAGS if f != "-fPIC"]


def _compile(src: Path, flags: list[str], out: Path) -> Path:
    # with --keep, a .s newer than its source and every header is reused
    newest = max(p.stat().st_mtime for p in [src, *src.parent.glob("*.h")])
    if out.exists() and out.stat().st_mtime >= newest:
        return out
    cmd = ["hipcc", *flags, "--cuda-device-only", "-S", str(src), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{res.stderr}")
    return out


def parse(asm: str) -> dict[str, dict]:
    """{function name: {"hist": Counter of mnemonics, "meta": {...} (kernels only)}}"""
    funcs: dict[str, dict] = {}
    is_func = set(re.findall(r"^\s*\.type\s+([\w.$]+),@function", asm, re.M))
    cur = None
    for line in asm.splitlines():
        m = re.match(r"^([\w.$]+):", line)
        if m and m.group(1) in is_func:
            cur = funcs.setdefault(m.group(1), {"hist": collections.Counter(), "meta": None})
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None or not line.startswith("\t"):
            continue
        tok = line.split(None, 1)
        if tok and tok[0][0] not in ".;":
            cur["hist"][tok[0]] += 1
    # metadata: the YAML note at the end; kernels are the items at two spaces of indent
    note = asm[asm.find("amdhsa.kernels:"):]
    for item in re.split(r"^  - ", note, flags=re.M)[1:]:
        kv = dict(re.findall(r"^(?:    )?(\.\w+):\s+(\S+)\s*$", item, re.M))
        name = kv.get(".name")
        if name in funcs:
            funcs[name]["meta"] = {k: kv.get(k, "0") for k in META_KEYS}
    return funcs


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent", type=Path)
    ap.add_argument("change", type=Path)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", type=Path, help="keep the .s files under this directory")
    ap.add_argument("--only", nargs="*", help="file stems to compare (default: all)")
    args = ap.parse_args()

    work = args.keep or Path(tempfile.mkdtemp(prefix="asm_compare_"))
    jobs = []
    for side, root in (("parent", args.parent), ("change", args.change)):
        flags = _flags(root)
        (work / side).mkdir(parents=True, exist_ok=True)
        for src in sorted((root / "pmarlo_amd/csrc").glob("*.hip")):
            if args.only and src.stem not in args.only:
                continue
            jobs.append((src, flags, work / side / (src.stem + ".s")))
    with ThreadPoolExecutor(max_workers=args.jobs) as pool:
        list(pool.map(lambda j: _compile(*j), jobs))

    bad = strict_bad = 0
    stems = sorted({j[2].stem for j in jobs})
    for stem in stems:
        sides = []
        for side in ("parent", "change"):
            p = work / side / (stem + ".s")
            sides.append(parse(p.read_text()) if p.exists() else {})
        a, b = sides
        n_k = sum(1 for f in a.values() if f["meta"])
        rows = []
        for name in sorted(set(a) | set(b)):
            if name not in a or name not in b:
                rows.append((name, "only in " + ("parent" if name in a else "change"), True))
                continue
            diffs = []
            if a[name]["meta"] != b[name]["meta"]:
                ma, mb = a[name]["meta"] or {}, b[name]["meta"] or {}
                diffs += [f"{k} {ma.get(k)}->{mb.get(k)}" for k in META_KEYS if ma.get(k) != mb.get(k)]
            ha, hb = a[name]["hist"], b[name]["hist"]
            strict = bool(diffs)
            for mn in sorted(set(ha) | set(hb)):
                if ha[mn] != hb[mn]:
                    diffs.append(f"{mn} {ha[mn]}->{hb[mn]}")
                    strict |= bool(STRICT.match(mn))
            if diffs:
                rows.append((name, ", ".join(diffs), strict))
        status = "identical" if not rows else f"{len(rows)} differ"
        print(f"{stem + '.hip':<18} {len(a):>3} functions ({n_k} kernels): {status}")
        for name, what, strict in rows:
            print(f"    {'DEFECT ' if strict else ''}{name}: {what}")
            bad += 1
            strict_bad += strict
    print(f"{bad} functions differ, {strict_bad} in resources or fp64/waitcnt/barrier counts; assembly in {work}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
