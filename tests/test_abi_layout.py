"""The ctypes mirrors of careless_amd/_lib.py against include/careless_hip.h, field by field: a C program generated from `_lib.ABI_STRUCTS`
prints `sizeof` of every argument struct and `offsetof` / `sizeof` of every mirrored field as g++ lays the header out; each value is compared
with the mirror's.  The load-time handshake (`cl_abi_sizeof`) compares total sizes only: two pointer fields swapped in a mirror pass it and
hand a kernel a wrong address.  Here a misspelt field does not compile, a swapped or retyped one fails the comparison, and a field the
mirror lacks leaves bytes of the struct that no mirrored field accounts for.  CPU only."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from careless_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "careless_hip.h")


def _program():
    lines = ["#include <stddef.h>", "#include <stdio.h>", f'#include "{HEADER}"', "int main(void) {"]
    for name, mirror in _lib.ABI_STRUCTS.items():
        lines.append(f'    printf("S {name} - %zu %zu\\n", (size_t)0, sizeof({name}));')
        for field, _ in mirror._fields_:
            lines.append(f'    printf("F {name} {field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
    return "\n".join(lines + ["    return 0;", "}", ""])


@pytest.fixture(scope="module")
def layout():
    """{struct: size}, {struct: [(field, offset, size), ...]} as the C++ compiler lays out the header"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tempfile.mkdtemp(prefix="cl_abi_")
    src, exe = os.path.join(d, "abi_layout.cpp"), os.path.join(d, "abi_layout")
    with open(src, "w") as f:
        f.write(_program())
    subprocess.check_call(["g++", "-O0", "-o", exe, src])
    sizes, fields = {}, {}
    for ln in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines():
        kind, struct, field, off, size = ln.split()
        if kind == "S":
            sizes[struct] = int(size)
        else:
            fields.setdefault(struct, []).append((field, int(off), int(size)))
    return sizes, fields


def test_every_argument_struct_of_the_header_has_a_mirror():
    with open(HEADER) as f:
        declared = set(re.findall(r"typedef struct (cl_\w+_args)\b", f.read()))
    assert declared == set(_lib.ABI_STRUCTS)


@pytest.mark.parametrize("name", list(_lib.ABI_STRUCTS))
def test_mirror_matches_the_header_field_by_field(layout, name):
    sizes, fields = layout
    mirror = _lib.ABI_STRUCTS[name]
    assert C.sizeof(mirror) == sizes[name]
    for field, off, size in fields[name]:
        m = getattr(mirror, field)
        assert (m.offset, m.size) == (off, size), f"{name}.{field}: mirror at {m.offset} (+{m.size}), header at {off} (+{size})"
    # the fields the sizes account for: walking the header's offsets, every byte of the struct is a mirrored field or the padding in front
    # of the next one's alignment (at the end: the struct's) -- so no field is missing from the mirror, and the count is the mirror's
    end, accounted = 0, 0
    for (field, off, size), (_, ctype) in zip(fields[name], mirror._fields_):
        assert off == -(-end // C.alignment(ctype)) * C.alignment(ctype), f"{name}: bytes {end} .. {off} in front of {field} belong to no mirrored field"
        end, accounted = off + size, accounted + 1
    assert sizes[name] == -(-end // C.alignment(mirror)) * C.alignment(mirror), f"{name}: bytes {end} .. {sizes[name]} belong to no mirrored field"
    assert accounted == len(mirror._fields_)
    # ... and the header's own declarators of the struct, counted in its text (a field small enough to hide in padding has nowhere to go)
    with open(HEADER) as f:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S), flags=re.S).group(1)
    declared = [re.sub(r"\[.*\]", "", d).split()[-1].lstrip("*") for stmt in body.split(";") if stmt.strip() for d in stmt.split(",")]
    assert declared == [f for f, _ in mirror._fields_]
