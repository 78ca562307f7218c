"""Side-by-side table of the compiler's kernel resource usage of two builds of libbohip.so.
Usage: resource_table.py PARENT.log THIS.log  -- each the stderr of the library's hipcc line with
-Rpass-analysis=kernel-resource-usage added (a cross-compile: no device needed).  Prints every kernel, VGPR / AGPR / scratch /
LDS / occupancy, parent beside this build, and marks the rows that differ; kernels are paired by name without their parameter
lists; exits 1 if a kernel gained scratch or lost occupancy."""
import re
import subprocess
import sys

KEYS = [("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"),
        ("Occupancy [waves/SIMD]", "occ")]


def short(name):
    try:
        d = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    except OSError:
        d = name
    d = re.sub(r"^void ", "", d).replace("bohip::", "")
    return re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", d)[:70]


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":   # (keyed without the parameter list: a kernel that lost a parameter is still that kernel)
            cur = out.setdefault(short(v), {})
        elif cur is not None:
            cur[k] = v
    return out


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    bad = 0
    print(f"{'kernel':70s} " + " ".join(f"{h + ' par/this':>16s}" for _, h in KEYS))
    for name in sorted(set(a) | set(b)):
        ra, rb = a.get(name), b.get(name)
        cells, diff = [], ra is None or rb is None
        for k, _ in KEYS:
            va, vb = (ra or {}).get(k, "-"), (rb or {}).get(k, "-")
            diff |= va != vb
            cells.append(f"{va + '/' + vb:>16s}")
        if ra and rb:
            if int(rb[KEYS[2][0]]) > int(ra[KEYS[2][0]]) or int(rb[KEYS[4][0]]) < int(ra[KEYS[4][0]]):
                bad += 1
        print(f"{name:70s} " + " ".join(cells) + ("   <-- differs" if diff else ""))
    print(f"\nkernels: parent {len(a)}, this build {len(b)}; gained scratch or lost an occupancy step: {bad}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
