"""Compare the device assembly of two builds of one .hip file, kernel by kernel.

    hipcc <FLAGS of esm_amd/build.py> -S --cuda-device-only old/x.hip -o old.s      (and new.s likewise)
    python tools/compare_device_asm.py old.s new.s [--drop-args KERNEL:I,J ...] [--diff N]

Kernels are paired by their demangled name; `--drop-args gemm9_kernel:2` removes template argument 2 (counted from 0)
of every old `gemm9_kernel<...>` before pairing — for a refactor that deleted a template parameter — and keeps only
the old instantiations whose dropped arguments have the value given after `=` (default 0 / false / 1 listed
explicitly: `gemm9_kernel:2=0`).  `--map-args layernorm_kernel:2:0=false,7=true` keeps the old instantiations whose
argument 2 is 0 or 7 and renames the value — for a parameter that changed its type.  Per pair it compares the `.amdhsa_*` resource block and the instruction stream after
replacing symbol names, basic-block label numbers and comments.  Prints one line per kernel and, for pairs that
differ, whether they are at least the same instructions up to register and label numbers (every s / v / a register, register
range and basic-block label masked), and the first N lines of a unified diff — of the masked streams where those differ, else of the plain ones.
"""
import argparse
import difflib
import re
import subprocess
import sys


def demangle(names):
    # binutils' c++filt does not know the _Float16 / __bf16 manglings: two other builtin types stand in for them
    stand_in = [n.replace("DF16_", "g").replace("DF16b", "e") for n in names]
    out = subprocess.run(["c++filt"], input="\n".join(stand_in), capture_output=True, text=True, check=True).stdout
    out = out.replace("__float128", "_Float16").replace("long double", "__bf16")
    return dict(zip(names, out.split("\n")))


def split_args(s):
    """Top-level comma split of a template argument list."""
    parts, depth, cur = [], 0, ""
    for ch in s:
        if ch in "<(":
            depth += 1
        elif ch in ">)":
            depth -= 1
        if ch == "," and depth == 0:
            parts.append(cur.strip())
            cur = ""
        else:
            cur += ch
    parts.append(cur.strip())
    return parts


def template_of(name):
    """'void ns::kern<a, b>(args)' -> ('ns::kern', [a, b]) ; names without template arguments -> (name, None)."""
    name = re.sub(r"^void ", "", name)
    name = name[: name.index("(")] if "(" in name and "<" not in name.split("(")[0] else name
    m = re.match(r"([\w:]+)<", name)
    if not m:
        return name.split("(")[0], None
    depth, i0 = 0, m.end()
    for i in range(m.end() - 1, len(name)):
        if name[i] == "<":
            depth += 1
        elif name[i] == ">":
            depth -= 1
            if depth == 0:
                return m.group(1), split_args(name[i0:i])
    return m.group(1), None


def parse(path):
    """{mangled kernel name: {"hsa": [lines], "code": [lines]}}"""
    text = open(path).read().split("\n")
    kernels, cur, hsa = {}, None, None
    names = set(re.findall(r"^\s*\.amdhsa_kernel (\S+)", "\n".join(text), re.M))
    for line in text:
        st = line.strip()
        m = re.match(r"^(\S+):", line)
        if m and m.group(1) in names:
            cur = m.group(1)
            kernels.setdefault(cur, {"hsa": [], "code": []})
            continue
        if st.startswith(".amdhsa_kernel "):
            hsa = st.split()[1]
            kernels.setdefault(hsa, {"hsa": [], "code": []})
            continue
        if st.startswith(".end_amdhsa_kernel"):
            hsa = None
            continue
        if hsa is not None:
            kernels[hsa]["hsa"].append(st)
            continue
        if cur is not None:
            if st.startswith(".Lfunc_end"):
                cur = None
                continue
            st = st.split(";")[0].rstrip()
            if not st or (st.startswith(".") and not st.endswith(":")):
                continue  # directives (alignment, CFI, ...) carry no instruction
            st = re.sub(r"\.LBB\d+_", ".LBB_", st)
            st = re.sub(r"_Z\w+", "SYM", st)
            st = re.sub(r"__hip_cuid_\w+", "CUID", st)
            kernels[cur]["code"].append(st)
    for k in kernels.values():  # basic-block labels numbered in the order in which the kernel defines them
        order = {}
        for l in k["code"]:
            m = re.match(r"(\.LBB_\d+):$", l)
            if m:
                order[m.group(1)] = f".L{len(order)}"
        k["code"] = [re.sub(r"\.LBB_\d+", lambda m: order.get(m.group(0), m.group(0)), l) for l in k["code"]]
    return kernels


def role_names(kernels, drops, maps={}):
    dm = demangle(list(kernels))
    roles = {}
    for mangled, full in dm.items():
        base, args = template_of(full)
        short = base.split("::")[-1]
        if args is not None and short in maps:
            idx, table = maps[short]
            if args[idx] not in table:
                roles[mangled] = None
                continue
            args[idx] = table[args[idx]]
        if args is not None and short in drops:
            keep = True
            for idx, val in drops[short]:
                if val is not None and args[idx] not in val:
                    keep = False
            if not keep:
                roles[mangled] = None
                continue
            args = [a for i, a in enumerate(args) if i not in [d[0] for d in drops[short]]]
        roles[mangled] = base + ("<" + ", ".join(args) + ">" if args is not None else "")
    return roles, dm


def mask_regs(lines):
    """Register and label numbers masked: the same opcodes, immediates and operand kinds remain."""
    return [re.sub(r"\.L\d+", ".L#", re.sub(r"\b([sva])(\d+|\[\d+:\d+\])", r"\1#", l)) for l in lines]


def hsa_compare(old, new):
    """-> list of differences; the SGPR count may only fall."""
    def as_map(lines):
        return {l.split()[0]: " ".join(l.split()[1:]) for l in lines if l.startswith(".amdhsa_")}
    a, b = as_map(old), as_map(new)
    out = []
    for k in sorted(set(a) | set(b)):
        if a.get(k) == b.get(k):
            continue
        if k == ".amdhsa_next_free_sgpr" and k in a and k in b and int(b[k]) <= int(a[k]):
            out.append(f"(allowed) {k} {a[k]} -> {b[k]}")
        else:
            out.append(f"{k} {a.get(k)} -> {b.get(k)}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--drop-args", nargs="*", default=[], help="KERNEL:I[=V|V2],J[=V] ... template arguments deleted by the refactor")
    ap.add_argument("--map-args", nargs="*", default=[], help="KERNEL:I:OLD=NEW,OLD=NEW ... a template argument that changed its values")
    ap.add_argument("--diff", type=int, default=60)
    a = ap.parse_args()
    drops = {}
    for d in a.drop_args:
        k, lst = d.split(":")
        drops[k] = []
        for item in lst.split(","):
            idx, _, val = item.partition("=")
            drops[k].append((int(idx), val.split("|") if val else None))
    maps = {}
    for d in a.map_args:
        k, idx, lst = d.split(":")
        maps[k] = (int(idx), dict(item.split("=") for item in lst.split(",")))
    old, new = parse(a.old), parse(a.new)
    r_old, dm_old = role_names(old, drops, maps)
    r_new, _ = role_names(new, {})
    by_role_new = {v: k for k, v in r_new.items()}
    gone = [dm_old[m] for m, r in r_old.items() if r is None or r not in by_role_new]
    same = differ = 0
    for m, r in sorted(r_old.items(), key=lambda kv: str(kv[1])):
        if r is None or r not in by_role_new:
            continue
        ko, kn = old[m], new[by_role_new[r]]
        hd = hsa_compare(ko["hsa"], kn["hsa"])
        hard = [x for x in hd if not x.startswith("(allowed)")]
        code_same = ko["code"] == kn["code"]
        if code_same and not hard:
            same += 1
            print(f"IDENTICAL  {r}  ({len(ko['code'])} lines){'  ' + '; '.join(hd) if hd else ''}")
        else:
            differ += 1
            mo, mn = mask_regs(ko["code"]), mask_regs(kn["code"])
            renamed = mo == mn
            nreg = sum(1 for x, y in zip(ko["code"], kn["code"]) if x != y) if renamed else 0
            print(f"DIFFERS    {r}  ({len(ko['code'])} -> {len(kn['code'])} lines)  resources: {'; '.join(hd) if hd else 'same'}"
                  + (f"  SAME INSTRUCTIONS, {nreg} lines differ in register numbers only" if renamed else ""))
            da, db = (ko["code"], kn["code"]) if renamed else (mo, mn)
            if not renamed:  # where the instructions differ: old line numbers of the first and the last changed block
                ops = [o for o in difflib.SequenceMatcher(None, mo, mn, autojunk=False).get_opcodes() if o[0] != "equal"]
                print(f"    instructions differ in old lines {ops[0][1] + 1} .. {ops[-1][2]} of {len(mo)} ({len(ops)} blocks)")
                tally = {}
                for _, i1, i2, j1, j2 in ops:
                    for l in mo[i1:i2] + mn[j1:j2]:
                        tally[l.split()[0]] = tally.get(l.split()[0], 0) + 1
                print("    removed + added lines by opcode: " + ", ".join(f"{k} {v}" for k, v in sorted(tally.items(), key=lambda kv: -kv[1])))
            for i, l in enumerate(difflib.unified_diff(da, db, "old", "new", n=2, lineterm="")):
                if i >= a.diff:
                    print("    ...")
                    break
                print("    " + l)
    added = [r for r in by_role_new if r not in set(r_old.values())]
    print(f"kernels: old {len(old)}, new {len(new)}; paired identical {same}, paired differing {differ}, gone {len(gone)}, new-only {len(added)}")
    for g in sorted(gone):
        print("GONE       " + g)
    for g in sorted(added):
        print("NEW-ONLY   " + g)
    return 1 if differ or added else 0


if __name__ == "__main__":
    sys.exit(main())
