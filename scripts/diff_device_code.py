"""Are the gfx950 kernels of two builds of libcareless_hip.so the same, instruction for instruction?  (No GPU needed.)

    python scripts/diff_device_code.py OLD.so NEW.so
    python scripts/diff_device_code.py --report OLD.so NEW.so      # every kernel: unchanged, or its registers / spills / scratch before -> after

A change that touches host code only -- or moves a device helper from one file to another -- must leave every kernel as it was: then the
speed of the kernels is the parent's by construction.  Both libraries are unbundled and disassembled (the tools of
scripts/check_lane_isa.py); kernels are matched by name (demangled where llvm-cxxfilt is installed), without the suffix the compiler
derives from the source path for kernels with internal linkage.  Compared per kernel: the instruction sequence (mnemonic and operands; addresses and the comments
derived from them are dropped, and so is the fill behind a kernel's last instruction) and the kernel descriptor's resources (register counts, scratch and LDS size).  Exit code 1 and one
line per kernel that is missing, extra or different.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys
import tempfile
from collections import defaultdict

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_lane_isa import OBJDUMP, demangle, parse_objdump, unbundle  # noqa: E402

READELF = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")
RESOURCES = (".sgpr_count", ".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count", ".private_segment_fixed_size",
             ".group_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size")
_UNIQUE = re.compile(r"\.(intern|static|anon)\.[0-9A-Za-z_]+|__[0-9a-f]{8,}(?=\b)")


def resources(co: str) -> dict:
    """mangled kernel name -> the resource fields of its entry in the code object's metadata note"""
    txt = subprocess.run([READELF, "--notes", co], stdout=subprocess.PIPE, text=True, check=True).stdout
    out, cur = {}, {}
    for ln in txt.split("\n"):
        m = re.match(r"\s*(?:- )?(\.[a-z_]+):\s*(\S+)\s*$", ln)
        if not m:
            continue
        if ln.lstrip().startswith("- ") and cur.get(".symbol"):      # the next kernel's record begins
            out[cur[".symbol"][:-len(".kd")]] = cur
            cur = {}
        cur[m.group(1)] = m.group(2).strip("'\"")
    if cur.get(".symbol"):
        out[cur[".symbol"][:-len(".kd")]] = cur
    return {k: tuple(v.get(f) for f in RESOURCES) for k, v in out.items()}


def _without_padding(texts: list) -> tuple:
    """The disassembler counts the `s_nop 0` fill behind a kernel's last instruction -- up to the next kernel's alignment, and a longer run
    behind the LAST kernel of a code object -- as that kernel's: how long the run is says where the kernel stands in its file, not what it
    executes (nothing behind its final `s_endpgm` or branch).  Dropped, so that a kernel moved to another file compares equal."""
    n = len(texts)
    while n > 0 and texts[n - 1] == "s_nop 0":
        n -= 1
    return tuple(texts[:n])


def kernels_of(lib: str) -> dict:
    """demangled name (path-derived suffix stripped) -> sorted list of (resources, instruction texts), one per code object that holds it"""
    out = defaultdict(list)
    with tempfile.TemporaryDirectory() as d:
        for co in unbundle(lib, d):
            txt = subprocess.run([OBJDUMP, "-d", co], stdout=subprocess.PIPE, text=True, check=True).stdout
            ks = {k: v for k, v in parse_objdump(txt).items() if v[1]}
            res = resources(co)
            for k, name in demangle(list(ks)).items():
                out[_UNIQUE.sub("", name)].append((res.get(k), _without_padding([i.text for i in ks[k][1]])))
    return {k: sorted(v, key=repr) for k, v in out.items()}


REPORT = (".vgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size")


def _family(name: str) -> str:
    """`elbo_lane_kernel` of a mangled (or demangled) kernel name: the identifier in front of the template or function arguments"""
    m = re.match(r"_ZN?(?:12_GLOBAL__N_1)?(\d+)", name)
    if m:
        return name[m.end():m.end() + int(m.group(1))]
    return re.split(r"[<(]", name.split("::")[-1])[0].split()[-1]


def report(old_lib: str, new_lib: str) -> int:
    """One line per kernel name: `=` (every copy unchanged instruction for instruction, resources included), `+` a kernel the new library
    adds, or `*` with the REPORT fields of every changed copy before -> after and its instruction counts; in front of them one `#` line of
    counts per kernel family.  Exit code 1 when a changed kernel gained spilled registers or scratch, or a kernel of the old library is missing."""
    from collections import Counter
    old, new = kernels_of(old_lib), kernels_of(new_lib)
    idx = [RESOURCES.index(f) for f in REPORT]
    worse, same, changed, added = [], [], [], []
    for k in sorted(set(old) | set(new)):
        if k not in old:
            for r1, i1 in new[k]:
                added.append(f"+ {k}: " + ", ".join(f"{n[1:]} {int(r1[i])}" for n, i in zip(REPORT, idx)) + f"; instructions {len(i1)}")
        elif k not in new or len(old[k]) != len(new[k]):
            worse.append(f"! {k}: missing from the new library, or another number of copies")
        elif old[k] == new[k]:
            same.append(k)
        else:
            for (r0, i0), (r1, i1) in zip(old[k], new[k]):
                if (r0, i0) == (r1, i1):
                    continue
                f0, f1 = [int(r0[i]) for i in idx], [int(r1[i]) for i in idx]
                changed.append(f"* {k}: " + ", ".join(f"{n[1:]} {a} -> {b}" for n, a, b in zip(REPORT, f0, f1)) + f"; instructions {len(i0)} -> {len(i1)}")
                if any(b > a for a, b in zip(f0[2:], f1[2:])):
                    worse.append(f"! {k}: gained spilled registers or scratch")
    print(f"# {len(same)} kernel names unchanged instruction for instruction (=), {len(changed)} changed copies (*), {len(added)} added (+), {len(worse)} findings (!)")
    for mark, names in (("=", same), ("*", [c[2:].split(":")[0] for c in changed]), ("+", [a[2:].split(":")[0] for a in added])):
        fam = Counter(_family(n) for n in names)
        print(f"# {mark} by family: " + (", ".join(f"{k} {v}" for k, v in sorted(fam.items())) or "none"))
    for ln in worse + changed + added + [f"= {k}" for k in same]:
        print(ln)
    return 1 if worse else 0


def main() -> int:
    if len(sys.argv) == 4 and sys.argv[1] == "--report":
        return report(sys.argv[2], sys.argv[3])
    if len(sys.argv) != 3:
        print(__doc__)
        return 2
    old, new = kernels_of(sys.argv[1]), kernels_of(sys.argv[2])
    bad = [f"only in {sys.argv[1]}: {k}" for k in sorted(set(old) - set(new))] + [f"only in {sys.argv[2]}: {k}" for k in sorted(set(new) - set(old))]
    for k in sorted(set(old) & set(new)):
        if old[k] == new[k]:
            continue
        if len(old[k]) != len(new[k]):
            bad.append(f"{k}: {len(old[k])} copies against {len(new[k])}")
            continue
        for (r0, i0), (r1, i1) in zip(old[k], new[k]):
            if r0 != r1:
                bad.append(f"{k}: resources {dict(zip(RESOURCES, r0 or ()))} against {dict(zip(RESOURCES, r1 or ()))}")
            if i0 != i1:
                at = next((n for n, (a, b) in enumerate(zip(i0, i1)) if a != b), min(len(i0), len(i1)))
                bad.append(f"{k}: {len(i0)} against {len(i1)} instructions, first difference at #{at}: "
                           f"`{i0[at] if at < len(i0) else '(end)'}` against `{i1[at] if at < len(i1) else '(end)'}`")
    for b in bad:
        print(b)
    n0, n1 = sum(len(v) for v in old.values()), sum(len(v) for v in new.values())
    print(f"{n0} kernels against {n1}: {len(bad)} differ")
    return 1 if bad or n0 != n1 else 0


if __name__ == "__main__":
    sys.exit(main())
