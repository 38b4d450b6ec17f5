"""Static opcode census of track_kernel, two trees side by side: the screen a change to csrc/tt_track.hip passes before
GPU time is spent on its bitwise dump (tools/track_dump.py).

    python tools/track_opcode_census.py OLD NEW [--keep DIR [--new-only]]

OLD and NEW are each a git revision or the root of a source tree.  tt_track.hip and tt_track_dual.hip of both are
compiled for the device only to assembly (about 40 s per tree).  Per track_kernel instantiation the tool prints the
count of every v_*_f64* and every ds_* opcode and the kernel's VGPR, AGPR, SGPR, spill, scratch, LDS and occupancy
figures, OLD beside NEW; it counts those two opcode families and nothing else.  A difference in the FP64 arithmetic
counts (fma, mul, add, rcp, min, max) is marked `<-- FP64`: a product was contracted differently, or an operation was
added or lost, and the bitwise dump will fail.  Exit status 1 if any instantiation is marked or is missing on one side.
--keep DIR leaves the four assembly files there; --new-only then reads OLD's assembly from DIR instead of rebuilding it
(the parent does not change between the steps of one refactor).
"""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from collections import Counter
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
HIPCC = "/opt/rocm/bin/hipcc"
UNITS = ("tt_track", "tt_track_dual")
# the FP64 arithmetic families; v_fmac is the fma whose addend register is its destination, the allocator's choice
ARITH = {"fma": ("v_fma_f64", "v_fmac_f64"), "mul": ("v_mul_f64",), "add": ("v_add_f64",), "rcp": ("v_rcp_f64",),
         "min": ("v_min_f64",), "max": ("v_max_f64",)}
META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")


def materialise(spec, tmp):
    """The tree root of `spec`: the directory itself, or csrc/ and include/ of that git revision under tmp."""
    if (Path(spec) / "car-trailer-mpc_amd" / "csrc").is_dir():
        return Path(spec)
    root = Path(tmp) / re.sub(r"\W", "_", spec)
    names = subprocess.run(["git", "ls-tree", "-r", "--name-only", spec, "car-trailer-mpc_amd/csrc/", "include/"],
                           cwd=REPO, check=True, capture_output=True, text=True).stdout.split()
    for n in names:
        (root / n).parent.mkdir(parents=True, exist_ok=True)
        (root / n).write_bytes(subprocess.run(["git", "show", f"{spec}:{n}"], cwd=REPO, check=True,
                                              capture_output=True).stdout)
    return root


def assemble(root, unit, out):
    csrc = root / "car-trailer-mpc_amd" / "csrc"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", f"-I{root / 'include'}", f"-I{csrc}",
                    "--cuda-device-only", "-S", str(csrc / f"{unit}.hip"), "-o", str(out)], check=True)
    return out


def census(path):
    """{instantiation: (Counter of opcodes, {figure: value})} of the track_kernel instantiations in an assembly file."""
    text = Path(path).read_text()
    out = {}
    for m in re.finditer(r"^(_Z\w*track_kernel\w*):[^\n]*\n(.*?)^\s*\.size\s+\1,", text, re.M | re.S):
        ops = Counter()
        for ln in m.group(2).splitlines():
            op = ln.split(None, 1)[0] if ln.strip() else ""
            if re.fullmatch(r"v_\w+_f64\w*", op) or op.startswith("ds_"):
                ops[re.sub(r"_e(32|64)$", "", op)] += 1
        occ = re.search(r"^; Occupancy: (\d+)", text[m.end():], re.M)
        out[m.group(1)] = [ops, {"occupancy": int(occ.group(1)) if occ else -1}]
    for blk in re.split(r"^  - \.agpr_count:", text, flags=re.M)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"^\s*\.name:\s+(\S+)", blk, re.M).group(1)
        if name in out:
            for k in META:
                out[name][1][k[1:]] = int(re.search(rf"^\s*\{k}:\s+(\d+)", blk, re.M).group(1))
    return {re.sub(r".*track_kernel(_dual)?ILi(n?\d+)ELi(\d+)ELi(\d+)E.*",
                   lambda g: f"{'dual' if g.group(1) else 'plain'}<{g.group(2).replace('n', '-')},{g.group(3)},{g.group(4)}>", k): v
            for k, v in out.items()}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    keep = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else None
    if keep:
        args.remove(keep)
    new_only = "--new-only" in sys.argv  # with --keep DIR: the OLD assembly already in DIR is read, not rebuilt
    old, new = args
    with tempfile.TemporaryDirectory() as tmp:
        dst = Path(keep) if keep else Path(tmp)
        dst.mkdir(parents=True, exist_ok=True)
        side = []
        for tag, spec in (("old", old), ("new", new)):
            fresh = not (new_only and tag == "old")
            root = materialise(spec, tmp) if fresh else None
            c = {}
            for u in UNITS:
                c.update(census(assemble(root, u, dst / f"{u}_{tag}.s") if fresh else dst / f"{u}_{tag}.s"))
            side.append(c)
    A, B = side
    marked = 0
    print(f"old = {old}   new = {new}")
    for inst in sorted(set(A) | set(B)):
        if inst not in A or inst not in B:
            print(f"\n== {inst}: only in {'old' if inst in A else 'new'}  <-- MISSING")
            marked += 1
            continue
        (oa, fa), (ob, fb) = A[inst], B[inst]
        fam = {f: (sum(oa[k] for k in ks), sum(ob[k] for k in ks)) for f, ks in ARITH.items()}
        bad = [f for f, (a, b) in fam.items() if a != b]
        marked += bool(bad)
        print(f"\n== {inst}" + (f"  <-- FP64 arithmetic differs: {', '.join(bad)}" if bad else "  FP64 arithmetic equal"))
        for k in sorted(set(fa) | set(fb)):
            print(f"  {k:28s} {fa.get(k, -1):8d} {fb.get(k, -1):8d}" + ("   *" if fa.get(k) != fb.get(k) else ""))
        for f, (a, b) in fam.items():
            print(f"  {'FP64 ' + f:28s} {a:8d} {b:8d}" + ("   <-- FP64" if a != b else ""))
        for k in sorted(set(oa) | set(ob)):
            print(f"  {k:28s} {oa[k]:8d} {ob[k]:8d}" + ("   *" if oa[k] != ob[k] else ""))
    print(f"\n{len(set(A) | set(B))} instantiations, {marked} marked")
    return 1 if marked else 0


if __name__ == "__main__":
    sys.exit(main())
