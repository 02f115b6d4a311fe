"""What the resource tests share: one csrc source compiled to gfx950 device assembly with the library's code generation
flags (no GPU: hipcc cross-compiles), and the resource lines the compiler writes after each kernel."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vlite-fast_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ("-O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt "
         "-fno-gpu-flush-denormals-to-zero -I../../include -I. -w --cuda-device-only -S -o -").split()
LINES = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")


def compile_usage(src):
    """src: a file name under csrc -> ({kernel symbol: {resource line: value}} over LINES, the assembly text)"""
    r = subprocess.run([HIPCC] + FLAGS + [src], cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    asm = r.stdout.decode()
    use, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            continue
        m = re.match(r"^; (%s): (\d+)" % "|".join(LINES), line)
        if m and cur:
            use.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    return use, asm


def kernel_text(asm, sym):
    """the instructions of the kernel whose symbol is sym: from its label to the end of its function"""
    start = asm.index("\n%s:" % sym)
    return asm[start:asm.index(".Lfunc_end", start)]
