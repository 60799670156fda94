#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, no GPU needed:  tools/kernel_diff.py A B [--rename old=new ...]

A and B are device ELFs, directories of device ELFs (*.elf), or source directories (*.hip + Makefile), which are
compiled device-only with the Makefile's own CXXFLAGS into a temporary directory.  Kernels are matched by demangled
name over the union of each side's files (so a kernel may move between translation units); --rename maps a name of A to
its name in B (substring replacement, e.g. 'score_pass1_dma_kernel<2, true, =score_pass1_dma_kernel<2, ').
Prints the kernels only in A, only in B, and those whose disassembly (addresses, symbol names and comments stripped) or
64-byte kernel descriptor (minus the code-entry offset, which moves with the layout) differ.  Exit status 1 if any differ.
"""
import argparse, difflib, glob, os, re, struct, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def compile_dir(src, tmp):
    flags = re.search(r"^CXXFLAGS\s*:?=\s*(.*)$", run("make", "-C", src, "-pn"), re.M).group(1).split()
    def one(f):
        out = os.path.join(tmp, os.path.basename(f)[:-4] + ".elf")
        run(HIPCC, *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-c", f, "-o", out)
        return out
    with ThreadPoolExecutor(int(os.environ.get("JOBS", "4"))) as ex:
        return list(ex.map(one, sorted(glob.glob(os.path.join(src, "*.hip")))))


def elf_kernels(path):
    """{demangled name: (normalised disassembly, descriptor bytes)} of one device ELF"""
    data = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<QQQ", data, shoff + i * shentsize + 0x10) for i in range(shnum)]   # addr, offset, size
    kd = {}
    for line in run("nm", path).splitlines():
        addr, _, name = line.split(None, 2) if line[0] != " " else ("", "", "")
        if name.endswith(".kd"):
            a = int(addr, 16)
            sa, so, _ = next(s for s in secs if s[0] <= a < s[0] + s[2] and s[0])
            d = bytearray(data[so + a - sa:so + a - sa + 64])
            d[16:24] = bytes(8)   # KERNEL_CODE_ENTRY_BYTE_OFFSET
            kd[name[:-3]] = bytes(d)
    body, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", path).splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = body.setdefault(m.group(1), [])
        elif cur is not None and line.strip() not in ("", "..."):   # ("...": zero padding after a section's last kernel)
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    for lines in body.values():   # alignment padding after the last instruction (a lone zero dword decodes as a v_cndmask)
        while lines and (lines[-1].split()[0] in ("s_nop", "s_code_end") or lines[-1].startswith("v_cndmask_b32_e32 v0, s0, v0")):
            lines.pop()
    names = sorted(kd)
    dem = run("c++filt", *names).splitlines() if names else []
    return {d: ("\n".join(body.get(n, [])), kd[n]) for n, d in zip(names, dem)}


def side(arg, tmp):
    if os.path.isdir(arg):
        files = sorted(glob.glob(os.path.join(arg, "*.elf"))) or compile_dir(arg, tmp)
    else:
        files = [arg]
    out, per_file = {}, {}
    for f in files:
        ks = elf_kernels(f)
        per_file[os.path.basename(f)] = len(ks)
        for n, v in ks.items():
            if out.setdefault(n, v) != v:
                sys.exit(f"{arg}: {n} is compiled differently in two files")
    return out, per_file


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a"), ap.add_argument("b")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N diff lines of each differing kernel")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        (ka, fa), (kb, fb) = side(args.a, ta), side(args.b, tb)
    for r in args.rename:
        old, new = r.split("=", 1)
        ka = {n.replace(old, new): v for n, v in ka.items()}
    for f in sorted(set(fa) | set(fb)):
        print(f"{f}: {fa.get(f, 0)} -> {fb.get(f, 0)} kernels")
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    differ = [(n, ka[n][0] != kb[n][0], ka[n][1] != kb[n][1]) for n in sorted(set(ka) & set(kb)) if ka[n] != kb[n]]
    for title, names in (("only in A", only_a), ("only in B", only_b)):
        print(f"{title}: {len(names)}")
        for n in names:
            print("   ", n)
    print(f"common: {len(set(ka) & set(kb))}, differ: {len(differ)}")
    for n, code, desc in differ:
        print("   ", n, "[code]" if code else "", "[descriptor]" if desc else "")
        d = difflib.unified_diff(ka[n][0].split("\n"), kb[n][0].split("\n"), "A", "B", n=2, lineterm="")
        print("\n".join(list(d)[:args.show]))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
