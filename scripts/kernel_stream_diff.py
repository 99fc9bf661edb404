"""Compare the gfx950 instruction streams of two builds of the library, kernel by kernel (device functions included): every symbol of the first
file must exist in the second with the same sequence of (opcode, operands) -- but for the literal of a pc-relative address (s_getpc_b64 followed by
s_add_u32 / s_addc_u32), which is the distance to a constant table and moves when code elsewhere grows.  Symbols only the second file has are
listed as new.  A function that several translation units emit (a non-template kernel or out-of-line device function of a shared header, each unit
with its own flags) has several copies under one name: every copy of the first file must be among the second file's, in whatever order the units
were linked.
usage: python scripts/kernel_stream_diff.py OLD.so NEW.so [--added-default VALUE]     (exit status 1 if a common symbol differs or one is missing)
--added-default VALUE: a template of NEW gained a trailing parameter whose default is VALUE (e.g. `false`), which renames every instantiation.  A
symbol of OLD that NEW lacks is then compared with NEW's symbol whose demangled name has `, VALUE` appended to the function's template arguments (the
parameter list is not compared), and counts as identical / differing under that name."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resources import extract_all

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def streams(path):
    """{mangled symbol: set of (instruction count, sha256 of its "opcode operands" lines), one per distinct copy} over every gfx950 code object of the file"""
    out, copies = {}, {}
    for co in extract_all(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co), f.flush()
            text = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
        cur, pcrel = None, 0
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                cur = m.group(1)
                out[cur] = [0, hashlib.sha256()]
                copies.setdefault(cur, []).append(out[cur])
                continue
            m = re.match(r"^\s+(\S+)\s*(.*?)\s*// [0-9A-F]+:", line)
            if m and cur:
                op, args = m.group(1), m.group(2)
                # s_getpc_b64 + s_add_u32 / s_addc_u32 <literal>: the distance from here to a constant table, which moves when code elsewhere grows
                if op == "s_getpc_b64":
                    pcrel = 2
                elif pcrel and op in ("s_add_u32", "s_addc_u32"):
                    args, pcrel = re.sub(r"(0x[0-9a-f]+|-?\d+)$", "<pc-relative>", args), pcrel - 1
                else:
                    pcrel = 0
                out[cur][0] += 1
                out[cur][1].update(f"{op} {args}\n".encode())
    return {k: {(n, h.hexdigest()) for n, h in v} for k, v in copies.items()}


def main():
    old, new = streams(sys.argv[1]), streams(sys.argv[2])
    if "--added-default" in sys.argv:
        value = sys.argv[sys.argv.index("--added-default") + 1]
        lacking, fresh = sorted(set(old) - set(new)), sorted(set(new) - set(old))
        plain = subprocess.run(["c++filt"], input="\n".join(lacking + fresh), capture_output=True, text=True).stdout.splitlines()
        # (by the name and its template arguments alone: a parameter type that depends on the new template parameter is spelt differently too)
        by_name = {name.split(">(", 1)[0]: k for name, k in zip(plain[len(lacking):], fresh)}
        renamed = 0
        for k, name in zip(lacking, plain):
            target = by_name.get(name.split(">(", 1)[0] + f", {value}") if ">(" in name else None
            if target is not None:
                new[k] = new.pop(target)
                renamed += 1
        print(f"{renamed} symbols of the first file compared under their name with `, {value}` appended to the template arguments")
    missing = sorted(set(old) - set(new))
    differ = sorted(k for k in old if k in new and not old[k] <= new[k])
    added = sorted(set(new) - set(old))
    print(f"{len(old)} symbols in {sys.argv[1]}, {len(new)} in {sys.argv[2]}: {len(old) - len(missing) - len(differ)} identical, "
          f"{len(differ)} differ, {len(missing)} missing, {len(added)} new ({sum(max(n for n, _ in new[k]) for k in added)} instructions)")
    names = subprocess.run(["c++filt"], input="\n".join(differ + missing + added), capture_output=True, text=True).stdout.splitlines()
    for tag, group in (("DIFFERS", differ), ("MISSING", missing), ("new", added)):
        for k in group:
            print(f"  {tag}: {names.pop(0)[:160]}")
    return 1 if (differ or missing) else 0


if __name__ == "__main__":
    sys.exit(main())
