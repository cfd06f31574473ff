#!/usr/bin/env python3
"""Fingerprints of the reference lines integration/kanzi-hip.patch is made against, for tests/test_abi.py::test_reference_patch_applies
(the reference's Java tree is not part of this repository).  For every hunk: its file, where its old side starts, how many lines
it spans, and the sha256 of those lines as they stand in the reference -- digests only, no reference text.
    tools/patch_preimage.py <reference checkout (the directory holding java/)> > tests/golden/reference_patch_preimage.json"""
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "integration", "kanzi-hip.patch")


def hunks(patch_text):
    """[(path relative to the tree root, old start, old count, old-side lines of the hunk)] of a unified diff"""
    out, path, cur = [], None, None
    for line in patch_text.splitlines():
        if line.startswith("--- a/"):
            path = line[len("--- a/"):].split("\t")[0]
        elif line.startswith("+++ ") or line.startswith("diff "):
            continue
        elif line.startswith("@@"):
            m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@", line)
            cur = (path, int(m.group(1)), int(m.group(2) or "1"), [])
            out.append(cur)
        elif cur is not None and line[:1] in (" ", "-"):
            cur[3].append(line[1:])
        elif cur is not None and line == "":
            cur[3].append("")                                          # a context line of an empty source line, its space stripped
    return out


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main():
    tree = sys.argv[1]
    res = {"patch": os.path.relpath(PATCH, ROOT), "hunks": []}
    for path, start, count, _ in hunks(open(PATCH).read()):
        with open(os.path.join(tree, path)) as f:
            src = f.read().splitlines()
        res["hunks"].append({"file": path, "old_start": start, "old_count": count, "file_lines": len(src),
                             "sha256": digest(src[start - 1:start - 1 + count])})
    json.dump(res, sys.stdout, indent=1)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
