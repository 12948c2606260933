#!/usr/bin/env python3
"""Digest of every kernel's gfx950 instructions in a library or object file (no GPU needed): one row per kernel,
sha256[:12]  instructions  demangled name, sorted by name.  Two builds whose tables are equal run the same device code,
which is how a refactor that must not touch the kernels is checked (diff the tables of the two trees).
The text hashed is llvm-objdump's disassembly of the kernel's symbol with the address-and-encoding comments cut off and
the literals of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 masked: those are distances to constant tables,
which move with the link, not instructions that differ.  Fill between functions (the s_nop / s_code_end run behind a
kernel's last instruction and objdump's "..." for zero bytes) depends on where the kernel lies in its unit and is left out.
  python tools/kernel_isa_digest.py [libvisomatch.so | unit.o] > table.txt"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "opencl-structure-from-motion_amd", "libvisomatch.so")
LLVM = "/opt/rocm/lib/llvm/bin"
SYM = re.compile(r"^(?:[0-9a-f]+ )?<(.+)>:$")
PCREL = re.compile(r"^(s_addc?_u32 \S+ \S+) (?:0x[0-9a-f]+|-?\d+|\S+@rel32@(?:lo|hi)\S*)$")  # a literal, never a register


def kernels_of(code_object):
    """names of the code object's kernels: every kernel has a descriptor symbol NAME.kd"""
    out = subprocess.run([LLVM + "/llvm-objdump", "-t", code_object], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1][:-3] for ln in out.splitlines() if ln.endswith(".kd")}


def bodies_of(code_object):
    """symbol -> its instruction lines, comments cut, pc-relative literals masked"""
    txt = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-leading-addr", "--no-show-raw-insn", code_object], check=True,
                         capture_output=True, text=True).stdout
    bodies, cur, since_getpc = {}, None, None
    for ln in txt.splitlines():
        m = SYM.match(ln.strip())
        if m:
            cur, since_getpc = bodies.setdefault(m.group(1), []), None
            continue
        ins = " ".join(ln.split("//")[0].replace(",", " ").split())
        if cur is None or not ins or ins == "...":
            continue
        if ins.startswith("s_getpc_b64"):
            since_getpc = 0
        elif since_getpc is not None:
            since_getpc += 1
            m = PCREL.match(ins)
            if m and since_getpc <= 2:
                ins = m.group(1) + " <pc-relative>"
            if since_getpc >= 2:
                since_getpc = None
        cur.append(ins)
    return bodies


rows = []
with tempfile.TemporaryDirectory() as td:
    tmp = os.path.join(td, "lib.so")
    os.symlink(os.path.abspath(lib), tmp)
    subprocess.run([LLVM + "/llvm-objdump", "--offloading", tmp], check=True, stdout=subprocess.DEVNULL, cwd=td)
    for fn in sorted(os.listdir(td)):
        if "amdgcn" not in fn or "gfx950" not in fn:
            continue
        co = os.path.join(td, fn)
        bodies = bodies_of(co)
        for k in kernels_of(co):
            name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(.*", "", name).replace("void ", "")
            body = bodies[k]
            while body and body[-1] in ("s_nop 0", "s_code_end"):
                body.pop()
            rows.append((name, hashlib.sha256("\n".join(body).encode()).hexdigest()[:12], len(body)))
for name, digest, n in sorted(rows):
    print("%s %6d  %s" % (digest, n, name))
