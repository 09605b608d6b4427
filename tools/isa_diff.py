#!/usr/bin/env python3
"""Compare the device assembly of two builds, function by function.

    make -C distributed_learning_simulator_amd/csrc asm     # in each tree: csrc/_build/*.s
    python tools/isa_diff.py OLD/_build NEW/_build

Each .s is split into functions (symbol label .. its .Lfunc_end), comments are
dropped and the function's index in its .LBBn_m labels is blanked, so a function
that only moved in its file compares equal.  Prints one of same / moved / DIFF /
gone / new per symbol and exits 1 on any DIFF; `moved` is a gone and a new symbol
of one file with equal bodies (a rename), and is no difference; the pairing blanks
every mangled name in a body, so it would not see a changed callee.  Text only: a
refactor's check that no surviving kernel changed.
"""
import os
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0]).strip()
        m = re.fullmatch(r"([A-Za-z_][\w$.]*):", line)
        if name is None and m and not line.startswith(".L"):
            name, body = m.group(1), []
        elif name is not None and re.fullmatch(r"\.Lfunc_end\d+:", line):
            out[name], name = body, None
        elif name is not None and line:
            body.append(line)
    return out


def main(old_dir, new_dir):
    count = {"same": 0, "moved": 0, "DIFF": 0, "gone": 0, "new": 0}
    names = lambda d: {f for f in os.listdir(d) if f.endswith(".s")}
    for fn in sorted(names(old_dir) | names(new_dir)):
        old, new = (functions(os.path.join(d, fn)) if os.path.exists(os.path.join(d, fn)) else {}
                    for d in (old_dir, new_dir))
        # a renamed function: a gone and a new symbol whose bodies are equal once the
        # mangled names in them (the kernel descriptor's, the next section's) are
        # blanked, paired once
        blank = lambda body: [re.sub(r"_Z\w+", "_Z", line) for line in body]
        fresh, moved = sorted(new.keys() - old.keys()), {}
        for sym in sorted(old.keys() - new.keys()):
            to = next((n for n in fresh if blank(new[n]) == blank(old[sym])), None)
            if to is not None:
                fresh.remove(to)
                moved[sym] = to
        for sym in sorted((old.keys() | new.keys()) - set(moved.values())):
            verdict = "moved" if sym in moved else "new" if sym not in old else \
                "gone" if sym not in new else "same" if old[sym] == new[sym] else "DIFF"
            count[verdict] += 1
            print(f"{verdict:5s}  {fn}  {sym}" + (f"  ->  {moved[sym]}" if sym in moved else ""))
    print("  ".join(f"{k}: {v}" for k, v in count.items()))
    return 1 if count["DIFF"] else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
