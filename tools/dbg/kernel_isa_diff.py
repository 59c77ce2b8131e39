"""Kernel-by-kernel comparison of the gfx950 code of two builds of libmp2gpu.so (no GPU needed):
    python tools/dbg/kernel_isa_diff.py OLD/libmp2gpu.so NEW/libmp2gpu.so [--show NAME]
Every kernel's disassembly (llvm-objdump -d --no-show-raw-insn --no-leading-addr, comments stripped) is hashed; kernels are matched
by demangled name without the argument list, so a kernel whose signature changed is still compared with its predecessor. Prints one
line per kernel that differs or exists on one side only -- instruction count, VGPRs and scratch bytes of both sides -- and a
summary. --show NAME prints a unified diff of that kernel's listings. Exit status 0 always: what may differ is the reader's call."""
import difflib, hashlib, os, re, shutil, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def short(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"\(anonymous namespace\)::", "", name.replace("mp2g::", ""))
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):  # the argument list: the first '(' outside template brackets
        if ch == "<": depth += 1
        elif ch == ">": depth -= 1
        elif ch == "(" and depth == 0: cut = i; break
    return name[:cut].replace("void ", "")


def kernels(lib):
    """{name: (listing lines, vgprs, scratch)} over all gfx950 code objects of the library"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)
        for f in sorted(x for x in os.listdir(d) if "gfx950" in x):
            path = os.path.join(d, f)
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], capture_output=True, text=True).stdout
            meta = {}
            for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                g = lambda k: (re.search(rf"\.{k}:\s+(\S+)", blk) or [None, "?"])[1]
                meta[g("name")] = (g("vgpr_count"), g("private_segment_fixed_size"))
            dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", path],
                                 capture_output=True, text=True, check=True).stdout
            cur = None
            for line in dis.splitlines():
                m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:$", line.strip())
                if m:
                    cur = m.group(1) if m.group(1) in meta else None
                    if cur:
                        name = short(cur)
                        while name in out: name += "'"  # the same name in two code objects
                        out[name] = ([], *meta[cur])
                        cur = name
                    continue
                line = re.sub(r"\s*(//|;).*$", "", line).strip()
                if cur and line: out[cur][0].append(re.sub(r"\s+", " ", line))
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    if "--show" in sys.argv:
        k = sys.argv[sys.argv.index("--show") + 1]
        print("\n".join(difflib.unified_diff(old.get(k, ([],))[0], new.get(k, ([],))[0], "old/" + k, "new/" + k, lineterm="", n=2)))
        return
    same = 0
    print(f"{'kernel':72s} {'insns':>13s} {'vgpr':>9s} {'scratch':>9s}")
    for k in sorted(set(old) | set(new)):
        a, b = old.get(k), new.get(k)
        if a and b and digest(a[0]) == digest(b[0]):
            same += 1
            continue
        col = lambda i: f"{a[i] if a else '-'}->{b[i] if b else '-'}"
        print(f"{k[:72]:72s} {(str(len(a[0])) if a else '-') + '->' + (str(len(b[0])) if b else '-'):>13s} {col(1):>9s} {col(2):>9s}")
    print(f"{len(old)} kernels in the old build, {len(new)} in the new one; {same} listings are byte-identical")


if __name__ == "__main__":
    main()
