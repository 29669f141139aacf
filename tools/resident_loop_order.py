"""Where the row loads and their waits stand in the loops of csrc/mdr_resident.hip, read off the assembly the product flags give.

    python tools/resident_loop_order.py [substring of a mangled kernel name ...]

Compiles the file for the device alone (no GPU needed) and prints, per inner loop of each kernel named (default: the benchmark's
k_rollout_resident<4,1,256,true> and one group form), the instructions per turn - vector / other - and the positions of the row
loads and of the waits, counted in instructions from the loop's label.  The rotated loops (profiles/r14_README.md section 5) hold
two trips per turn; in each trip the wait must stand a few instructions IN FRONT of the load, so that a load is in flight for a
whole trip:  loads [27, 102]  waits [25, 99].  A load at the top of a trip with its wait behind it, or a wait right behind a load,
means a compiler or a source change has undone the order that row_arrived / row_ahead are there to hold.  Nothing checks this in
the test suite: the results are the same bits either way, only the time differs."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT = ("k_rollout_residentILi4ELi1ELi256ELb1EE", "k_rollout_resident_groupILi8ELi4ELb1EE")


def loops(lines, pattern):
    start = [n for n, l in enumerate(lines) if re.match(r"^_ZN3mdr\S*:", l) and pattern in l][0]
    end = next(n for n in range(start + 1, len(lines)) if lines[n].startswith(".Lfunc_end"))
    n = start
    while n < end:
        if "Inner Loop Header" in lines[n]:
            label, m, vector, other, count, loads, waits = lines[n].split(":")[0], n + 1, 0, 0, 0, [], []
            while m < end:
                t = lines[m].strip()
                if t and not t.startswith(";") and not t.startswith("."):
                    count += 1
                    if t.startswith("v_") or t.startswith("global_"):
                        vector += 1
                    else:
                        other += 1
                    if t.startswith("s_waitcnt"):
                        waits.append(count)
                    if t.startswith("s_load") or t.startswith("global_load"):
                        loads.append(count)
                if re.search(r"cbranch\S*\s+" + re.escape(label) + "$", t):
                    break
                m += 1
            yield vector, other, loads, waits
            n = m
        n += 1


def main():
    from mdr_amd import build
    src = "mdr_resident.hip"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "mdr_resident.s")
        flags = [f for f in build.FLAGS if f != "-fPIC"] + list(build.SOURCE_FLAGS.get(src, ()))
        subprocess.run([build._hipcc(), *flags, "--cuda-device-only", "-S", src, "-o", out], cwd=build.CSRC, check=True, stderr=subprocess.DEVNULL)
        with open(out) as f:
            lines = f.read().split("\n")
    for pattern in sys.argv[1:] or DEFAULT:
        print(pattern)
        for vector, other, loads, waits in loops(lines, pattern):
            print("    per turn: %d vector, %d other; loads %s  waits %s" % (vector, other, loads, waits))


if __name__ == "__main__":
    main()
