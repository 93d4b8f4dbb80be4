#!/usr/bin/env python3
"""Compare the device code of two builds symbol by symbol: for a refactor that moves kernels between units without changing them.

    kernel_diff.py --before OLD.o [OLD2.o ...] --after NEW.o [NEW2.o ...] [--json OUT.json]

Each argument is a device-only code object (hipcc ... --offload-device-only --no-gpu-bundle-output -c unit.hip).  Every function
symbol of the `before` objects must exist exactly once across the `after` objects, with byte-identical instructions and identical
resource notes (registers, LDS, private segment, spills).  Exit status 0 when all of them do."""
import argparse
import hashlib
import json
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin/"
NOTE_KEYS = (".vgpr_count", ".sgpr_count", ".agpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
             ".vgpr_spill_count", ".sgpr_spill_count", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, stdout=subprocess.PIPE, text=True).stdout


def load(path):
    """{symbol: (sha256 of its bytes, size)}, {kernel: notes}, sha256 of .text"""
    text_addr = text_off = text_size = None
    for line in run(LLVM + "llvm-readelf", "-S", "-W", path).splitlines():
        m = re.match(r"\s*\[\s*\d+\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", line)
        if m:
            text_addr, text_off, text_size = (int(x, 16) for x in m.groups())
    blob = open(path, "rb").read()
    text = blob[text_off:text_off + text_size]
    funcs = {}
    for line in run(LLVM + "llvm-readelf", "-s", "-W", path).splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            addr, size = int(f[1], 16), int(f[2])
            body = text[addr - text_addr:addr - text_addr + size]
            assert len(body) == size, (path, f[7])
            funcs[f[7]] = (hashlib.sha256(body).hexdigest(), size)
    notes, cur = {}, None
    for line in run(LLVM + "llvm-readelf", "--notes", path).splitlines():
        # the metadata is YAML: a kernel's entry opens with "  - .key:", its own keys sit at four columns
        m = re.match(r"  (?:- |  )(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        key, val = m.groups()
        if line.startswith("  - "):
            cur = {}
        if cur is None:
            continue
        if key in NOTE_KEYS:
            cur[key] = val.strip()
        if key == ".name":
            notes[val.strip()] = cur
    return funcs, notes, hashlib.sha256(text).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--before", nargs="+", required=True)
    ap.add_argument("--after", nargs="+", required=True)
    ap.add_argument("--json")
    a = ap.parse_args()
    before = {p: load(p) for p in a.before}
    after = {p: load(p) for p in a.after}
    rows, bad = [], 0
    for p, (funcs, notes, _) in before.items():
        for name, (digest, size) in sorted(funcs.items()):
            homes = [q for q, (f2, _, _) in after.items() if name in f2]
            row = {"symbol": name, "bytes": size, "before": p, "after": homes}
            if len(homes) != 1:
                row["verdict"] = "missing" if not homes else "duplicated"
            else:
                f2, n2, _ = after[homes[0]]
                same_code = f2[name] == (digest, size)
                same_notes = notes.get(name) == n2.get(name)
                row["notes"] = notes.get(name)
                row["verdict"] = "identical" if same_code and same_notes else ("code differs" if not same_code else "notes differ")
                if not same_notes:
                    row["notes_after"] = n2.get(name)
            bad += row["verdict"] != "identical"
            rows.append(row)
    out = {"text_sha256": {"before": {p: v[2] for p, v in before.items()}, "after": {p: v[2] for p, v in after.items()}},
           "symbols": len(rows), "kernels_with_notes": sum(1 for r in rows if r.get("notes")), "not_identical": bad, "rows": rows}
    if a.json:
        json.dump(out, open(a.json, "w"), indent=1)
    for r in rows:
        if r["verdict"] != "identical":
            print(r["verdict"], r["symbol"], r["after"])
    print("%d symbols, %d with resource notes, %d not identical" % (len(rows), out["kernels_with_notes"], bad))
    for side in ("before", "after"):
        for p, h in out["text_sha256"][side].items():
            print(side, p, ".text sha256", h)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
