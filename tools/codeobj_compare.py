"""Are the kernels of two libvqa.so builds the same machine code? (dev tool for refactors that move kernels between
translation units)
    python tools/codeobj_compare.py OLD.so NEW.so
Per kernel symbol of every gfx950 code object: the instruction text with addresses and encodings stripped
(tools/kernel_diff.py's form of check_isa.disassemble()) and the descriptor facts of the code object notes (VGPR / SGPR
/ AGPR counts, LDS, private segment, spills, wavefront size, max workgroup size). Prints every kernel that exists
on one side only or differs; exit status 0 only when the sets and every kernel match."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_diff  # noqa: E402  (puts csrc on the path and imports check_isa)
from kernel_diff import check_isa  # noqa: E402

FACTS = ("vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
         "vgpr_spill_count", "sgpr_spill_count", "wavefront_size", "max_flat_workgroup_size", "kernarg_segment_size",
         "uses_dynamic_stack")


def notes(lib):
    """{kernel name: {fact: value}} from the amdhsa.kernels metadata of every gfx950 code object."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for i, (triple, blob) in enumerate(check_isa.code_objects(check_isa.fatbin(lib))):
            if not (triple.endswith("gfx950") and blob):
                continue
            f = os.path.join(d, f"co{i}.o")
            with open(f, "wb") as fh:
                fh.write(blob)
            text = subprocess.run([os.path.join(check_isa.LLVM, "llvm-readelf"), "--notes", f], capture_output=True,
                                  text=True, check=True).stdout
            # one "  - .args:" ... block per kernel; keys are sorted, so .name follows the facts before it
            for block in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
                block = ".agpr_count:" + block
                kv = dict(re.findall(r"\.(\w+):\s+(\S+)", block))
                m = re.search(r"\.name:\s+(\S+)", block)
                if m:
                    out[m.group(1)] = {k: kv.get(k) for k in FACTS}
    return out


def code(ins):
    """A kernel's instructions without what pads the section behind it: "..." (llvm-objdump's elision of zero bytes) and
    the s_nop / s_code_end run after the last instruction, whose length depends on what follows the kernel in its code
    object (the last kernel of a unit carries the whole end-of-section pad), not on the kernel."""
    ins = [i for i in ins if i != "..."]
    while ins and ins[-1] in ("s_nop 0", "s_code_end"):
        ins.pop()
    return ins


def main():
    old, new = sys.argv[1], sys.argv[2]
    ta, tb = ({k: code(v) for k, v in kernel_diff.funcs(lib).items()} for lib in (old, new))
    na, nb = notes(old), notes(new)
    kernels = sorted(set(na) | set(nb))
    bad = 0
    for name in kernels:
        if name not in na or name not in nb:
            print(f"only {'new' if name not in na else 'old'}: {name}")
            bad += 1
            continue
        why = []
        if ta.get(name) != tb.get(name):
            why.append(f"instructions ({len(ta.get(name) or [])} -> {len(tb.get(name) or [])})")
        why += [f"{k} {na[name][k]} -> {nb[name][k]}" for k in FACTS if na[name][k] != nb[name][k]]
        if why:
            print(f"differs: {name}: " + ", ".join(why))
            bad += 1
    print(f"{len(kernels)} kernels, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
