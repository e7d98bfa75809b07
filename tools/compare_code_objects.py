#!/usr/bin/env python3
"""Did a change leave the kernels it was not about alone?  Disassembles every gfx950 code object of two builds of a library
(`llvm-objdump -d`, no GPU needed) and compares them function by function: the instruction text, without addresses, encodings and the
symbol+offset comments (those move with the layout of the code object).

    python tools/compare_code_objects.py OLD/libroboy_sim.so [gym_roboy_amd/csrc/libroboy_sim.so]

Prints N of N functions of OLD identical, then the names that differ, are gone, or are new; exit code 1 if one differs or is gone."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import code_object_meta as com  # noqa: E402


def functions(lib_path):
    """{mangled symbol: [instruction text, ...]} over every gfx950 code object of the library"""
    out = {}
    for image in com.code_objects(lib_path):
        with tempfile.NamedTemporaryFile(suffix=".co") as fh:
            fh.write(image)
            fh.flush()
            text = subprocess.run([os.path.join(com.LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", fh.name],
                                  capture_output=True, text=True, check=True).stdout
        cur = None
        for line in text.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
            if m:
                cur = out.setdefault(m.group(1), [])
                continue
            if cur is None or not line.startswith("\t"):
                continue
            cur.append(re.sub(r"\s+", " ", line.split("//", 1)[0]).strip())
    for body in out.values():               # (the padding behind a function's last instruction belongs to the layout)
        while body and body[-1] in ("s_nop 0", "..."):
            body.pop()
    return out


def main():
    old = functions(sys.argv[1])
    new = functions(sys.argv[2] if len(sys.argv) > 2 else os.path.join(com.ROOT, "gym_roboy_amd", "csrc", "libroboy_sim.so"))
    same = [k for k in old if k in new and old[k] == new[k]]
    differ = [k for k in old if k in new and old[k] != new[k]]
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    print("%d of %d functions of the old build identical; %d differ, %d gone, %d new" % (len(same), len(old), len(differ), len(gone), len(added)))
    names = com.demangle(differ + gone + added)
    for what, keys in (("differs", differ), ("gone", gone), ("new", added)):
        for k in keys:
            print("  %-8s %s" % (what, com.short(names[k])))
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main())
