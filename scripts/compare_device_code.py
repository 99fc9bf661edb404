#!/usr/bin/env python3
"""Is the gfx950 device code of two builds the same?

    python scripts/compare_device_code.py OLD NEW

Objects and shared libraries (anything that carries offload bundles): the .text, .rodata and .note sections of every gfx950 code object, byte for
byte, the code objects paired in file order.  Whole files are not compared: clang embeds an id derived from the unit's path in the symbol table.
Assembly (`hipcc --cuda-device-only -S`, *.s): per function.  Every function in both files must have the same text (kernels: with their
.amdhsa_kernel block) and kernels the same metadata entry; the only normalisation is the function index inside local labels (.LBB<n>_,
.Lfunc_end<n>, .LJTI<n>_), which shifts when a function before it left.  In the text after a `;` -- comments, never code -- the same labels are
spelt BB<n>_, and a label line's comment is padded to a column, so a shorter index moves the padding: both are treated likewise, there only.  Functions only in OLD are listed by name; a function only in NEW fails.
Exit status 0: the same."""
import os
import re
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import extract_all  # noqa: E402

SECTIONS = (".text", ".rodata", ".note")


def elf_sections(co):
    """{name: bytes} of an ELF64 little-endian image"""
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", co, 0x3A)
    heads = [struct.unpack_from("<IIQQQQIIQQ", co, shoff + i * shentsize) for i in range(shnum)]
    names = heads[shstrndx]
    out = {}
    for h in heads:
        name = co[names[4] + h[0]:co.index(b"\0", names[4] + h[0])].decode()
        out[name] = b"" if h[1] == 8 else co[h[4]:h[4] + h[5]]  # SHT_NOBITS has no bytes
    return out


def compare_objects(old, new):
    a, b = extract_all(old), extract_all(new)
    bad = len(a) != len(b)
    print(f"gfx950 code objects: {len(a)} / {len(b)}")
    for k, (x, y) in enumerate(zip(a, b)):
        sx, sy = elf_sections(x), elf_sections(y)
        for name in SECTIONS:
            same = sx.get(name) == sy.get(name)
            bad |= not same
            print(f"  code object {k} {name:8} {len(sx.get(name, b'')):>9} / {len(sy.get(name, b'')):>9} bytes  {'identical' if same else 'DIFFERENT'}")
    return bad


LABEL = re.compile(r"(\.LBB|\.Lfunc_end|\.LJTI)\d+")
COMMENT_LABEL = re.compile(r"\b(BB)\d+(?=_)")  # how a loop comment names .LBB<n>_<m>


def normalise(line):
    """the line with the function index taken out of its local labels"""
    code, semi, comment = line.partition(";")
    code, n = LABEL.subn(r"\1#", code)
    if semi and n:
        code = code.rstrip(" ") + " "  # (the padding in front of a label line's comment)
    return code + semi + COMMENT_LABEL.sub(r"\1#", LABEL.sub(r"\1#", comment))


def functions(path):
    """({name: normalised text from its label to .Lfunc_end}, {kernel name: metadata entry}) of an AMDGPU assembly file"""
    lines = open(path).read().split("\n")
    funcs, cur, name = {}, None, None
    for ln in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            assert cur is None, f"{path}: {name} has no .Lfunc_end"
            name, cur = m.group(1), []
        elif cur is not None:
            cur.append(normalise(ln))
            if cur[-1].startswith(".Lfunc_end#:"):
                funcs[name], cur = "\n".join(cur), None
    assert cur is None, f"{path}: {name} has no .Lfunc_end"
    meta, at = {}, lines.index("amdhsa.kernels:") + 1
    entry = []
    for ln in lines[at:] + ["  - "]:
        if ln.startswith("  - ") or not ln.startswith("    "):
            if entry:
                meta[next(e.split()[1] for e in entry if e.strip().startswith(".name:") and not e.startswith("      "))] = "\n".join(entry)
            entry = []
            if not ln.startswith("  - "):
                break
        entry.append(ln)
    assert funcs and meta, f"{path}: no functions found"
    return funcs, meta


def compare_assembly(old, new):
    (fa, ma), (fb, mb) = functions(old), functions(new)
    gone, added = [n for n in fa if n not in fb], [n for n in fb if n not in fa]
    differ = [n for n in fa if n in fb and (fa[n] != fb[n] or ma.get(n) != mb.get(n))]
    print(f"functions: {len(fa)} / {len(fb)} (kernels {len(ma)} / {len(mb)}); in both and identical: {len(fa) - len(gone) - len(differ)}")
    for title, names in (("only in OLD", gone), ("only in NEW", added), ("DIFFERENT", differ)):
        for n in names:
            print(f"  {title}: {n}{' (kernel)' if n in ma or n in mb else ''}")
    return bool(added or differ)


def main():
    old, new = sys.argv[1:3]
    bad = compare_assembly(old, new) if old.endswith(".s") else compare_objects(old, new)
    print("SAME" if not bad else "NOT THE SAME")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
