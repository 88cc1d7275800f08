"""Compare the gfx950 kernels of two builds of libmlimgsynth_amd.so instruction by instruction.

usage: python3 tools/kernel_disasm_diff.py OLD.so NEW.so

Every offload bundle of the .hip_fatbin section is unbundled and disassembled; each kernel symbol of OLD must appear in NEW with the same
instruction stream.  PC-relative address constants (s_getpc_b64 + s_add_u32 / s_addc_u32) are masked: they move with the code layout.
Kernels that gained a trailing template parameter whose default keeps the old code (WRAP of gemm_kernel, gemm_skinny_kernel,
conv_smalln_kernel) are matched by their name with that default value.  Exit status 1 if any old kernel is missing or differs."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TRAILING = re.compile(r"^(void \(anonymous namespace\)::(gemm_kernel|gemm_skinny_kernel|conv_smalln_kernel)<.*), (false|0)>\((.*)$")


def kernels(so, tmp):
    fat = os.path.join(tmp, "fatbin")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", so, os.path.join(tmp, "stripped")], check=True)
    data = open(fat, "rb").read()
    offs = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = {}
    for i, o in enumerate(offs):
        bundle, co = os.path.join(tmp, f"b{i}"), os.path.join(tmp, f"b{i}.co")
        with open(bundle, "wb") as f:
            f.write(data[o:offs[i + 1] if i + 1 < len(offs) else len(data)])
        r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                            f"--input={bundle}", f"--output={co}"], capture_output=True)
        if r.returncode or not os.path.getsize(co):
            continue
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^([0-9a-f]+ )?<(.+)>:$", line.strip())
            if m:
                cur = m.group(2)
                out[cur] = []
                continue
            if not cur or not line.strip() or line.startswith("Disassembly"):
                continue
            s = re.sub(r"<[^>]*>", "<L>", re.sub(r"\s*//.*$", "", line).strip())
            prev = out[cur][-1] if out[cur] else ""
            pcrel = prev.startswith("s_getpc") or (s.startswith("s_addc_u32") and prev.startswith("s_add_u32") and "X" in prev)
            if (s.startswith(("s_add_u32", "s_addc_u32")) and pcrel) or "rel32" in s:
                s = re.sub(r"0x[0-9a-f]+", "X", s)
            out[cur].append(s)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, r))


def main():
    old_so, new_so = sys.argv[1:3]
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        a, b = kernels(old_so, t1), kernels(new_so, t2)
    da, db = demangle(list(a)), demangle(list(b))
    by_name = {TRAILING.sub(r"\1>(\4", db[k]): k for k in b}
    same, bad = 0, []
    for k, ins in a.items():
        kb = by_name.get(da[k])
        if kb is None:
            bad.append(("missing", da[k]))
        elif b[kb] != ins:
            bad.append(("differs", da[k]))
        else:
            same += 1
    for what, name in bad:
        print(what, name)
    print(f"old kernels {len(a)}, new kernels {len(b)}: {same} identical, {len(bad)} missing or different")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
