#!/usr/bin/env python
"""Per-kernel instruction text of the four render units, tiles.hip and
mesh.hip, this tree against a git revision:  tools/asm_compare.py [rev] [--keep DIR]
(--keep DIR leaves the assembly in DIR and reuses the revision's from there)

Each unit is compiled device-only to gfx950 assembly with its flags from
sdf3d_amd/build.py, once from `rev` (default HEAD) and once from the working
tree, and compared per kernel symbol with labels, comments and directives
dropped; the device functions the kernels call out of line (the library log
and pow fall-backs) are compared the same way.  Identical text settles a
kernel's behaviour and speed.  Prints one line per unit (kernels, identical,
differing; device functions), the names that differ and whether the symbols'
order in the code object moved; exit status 1 when anything differs.  Needs
no GPU.
"""
from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from sdf3d_amd import build  # noqa: E402

KERNEL_UNITS = ["render_exact.hip", "render_fast.hip", "render_exact_bulb.hip",
                "render_fast_bulb.hip", "tiles.hip", "mesh.hip"]


def assemble(tree: Path, unit: str, out: Path, reuse: bool = False) -> Path:
    s = out / (Path(unit).stem + ".s")
    if reuse and s.exists():
        return s
    subprocess.run([build._hipcc(), *build.COMMON, *dict(build.UNITS)[unit], "-I", tree / "sdf3d_amd" / "build",
                    "--cuda-device-only", "-S", tree / "sdf3d_amd" / "csrc" / unit, "-o", s], check=True)
    return s


def functions(asm: Path) -> tuple[dict[str, list[str]], set[str]]:
    """{function symbol: its instruction lines}, from `sym:` to its
    .Lfunc_end, in the file's order, and which of them are kernels."""
    text = asm.read_text()
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    names = kernels | set(re.findall(r"^\s*\.type\s+(\S+),@function", text, re.M))
    out: dict[str, list[str]] = {}
    cur = None
    for line in text.splitlines():
        line = re.sub(r"\s*;.*", "", line).strip()
        if not line:
            continue
        if line.endswith(":"):
            if line[:-1] in names:
                cur = out.setdefault(line[:-1], [])
            continue
        if line.startswith(".Lfunc_end") or line.startswith(".section"):
            cur = None
        if cur is None or line.startswith("."):
            continue
        # branch targets are labels: keep the mnemonic, drop the label's number
        cur.append(re.sub(r"\.L([A-Za-z_]+)[0-9_]+", r".L\1", line))
    return out, kernels


def main() -> int:
    args = sys.argv[1:]
    keep = None
    if "--keep" in args:
        i = args.index("--keep")
        keep = Path(args[i + 1])
        del args[i:i + 2]
    rev = args[0] if args else "HEAD"
    with tempfile.TemporaryDirectory() as tmp:
        base = Path(keep) if keep else Path(tmp)
        old_tree = Path(tmp) / "old"
        old_tree.mkdir()
        if not (keep and all((base / "old" / (Path(u).stem + ".s")).exists() for u in KERNEL_UNITS)):
            tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "sdf3d_amd", "include"],
                                 check=True, capture_output=True).stdout
            subprocess.run(["tar", "-x", "-C", old_tree], input=tar, check=True)
            (old_tree / "sdf3d_amd" / "build").mkdir(exist_ok=True)
        build.OBJ.mkdir(parents=True, exist_ok=True)
        jobs = []
        with ThreadPoolExecutor(8) as ex:
            for side, tree in (("old", old_tree), ("new", ROOT)):
                (base / side).mkdir(parents=True, exist_ok=True)
                for u in KERNEL_UNITS:
                    jobs.append((side, u, ex.submit(assemble, tree, u, base / side,
                                                   side == "old" and keep is not None)))
        asm = {(side, u): f.result() for side, u, f in jobs}
        bad = 0
        for u in KERNEL_UNITS:
            (old, old_k), (new, new_k) = functions(asm["old", u]), functions(asm["new", u])
            differ = sorted(k for k in old.keys() | new.keys() if old.get(k) != new.get(k))
            bad += len(differ)
            kd = [k for k in differ if k in old_k | new_k]
            line = (f"{u}: {len(new_k)} kernels, {len(new_k) - len([k for k in kd if k in new_k])} "
                    f"identical, {len(kd)} differ")
            if len(old) > len(old_k) or len(new) > len(new_k):
                line += (f"; device functions {len(new) - len(new_k)}, "
                         f"{len(differ) - len(kd)} differ")
            print(line)
            if list(old) != list(new):
                bad += 1
                print("  symbol order differs")
            for k in differ:
                what = ("only in " + ("old" if k in old else "new") if k not in old or k not in new
                        else f"{len(old[k])} -> {len(new[k])} instructions")
                print(f"  {k}: {what}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
