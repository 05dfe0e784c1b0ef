"""sha256 of every unit's filtered device assembly (csrc `make asm asm-diag`).

A change that must leave the GPU code alone is checked by building the .s
files of two commits and comparing these digests unit by unit:

    make -C rave_amd/csrc asm asm-diag BUILD=build_asm
    python tools/asm_digest.py rave_amd/csrc/build_asm > head.json

The filter drops what depends on the source text rather than on the code:
`.file` and `.ident` directives and every line naming `__hip_cuid_` (a hash of
the translation unit's source).
"""
import hashlib
import json
import os
import re
import sys

FILTER = r"^\s*\.(file|ident)\b|__hip_cuid_"
_DROP = re.compile(FILTER)


def digest(path: str) -> str:
    h = hashlib.sha256()
    with open(path, "r", encoding="utf-8", errors="surrogateescape") as f:
        for line in f:
            if not _DROP.search(line):
                h.update(line.encode("utf-8", errors="surrogateescape"))
    return h.hexdigest()


def digests(build_dir: str) -> dict:
    return {n[:-2]: digest(os.path.join(build_dir, n)) for n in sorted(os.listdir(build_dir)) if n.endswith(".s")}


if __name__ == "__main__":
    json.dump({"filter_drop_lines_matching": FILTER, "units": digests(sys.argv[1])}, sys.stdout, indent=1)
    print()
