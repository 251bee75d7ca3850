#!/bin/bash
# Did a change of the host plumbing or of a header reach the kernels?  Compiles kernel files of two trees (default: the four
# chain-kernel files; FILES: names without .hip, e.g. "mpp_maps mpp_train mpp_resample") to gfx950 assembly with build.py's flags,
# side by side, and prints per kernel the number of differing assembly lines and the register / scratch / LDS figures of its
# metadata (parent -> this where they differ):
#   bash profiles/tools/codeobj_diff.sh PARENT_TREE THIS_TREE [OUT_DIR [FILES]]
# PARENT_TREE: a checkout of the parent commit (git worktree add --detach ../parent HEAD~1).  The trees' paths enter the
# assembly through the __hip_cuid_* symbols only: lines containing __hip_cuid are dropped.  With OUT_DIR the .s files are
# kept there (and an existing OUT_DIR/parent is reused, not compiled again).  Exit status 1 when any line differs.
set -e
[ $# -ge 2 ] || { echo "usage: $0 PARENT_TREE THIS_TREE [OUT_DIR [FILES]]" >&2; exit 2; }
parent=$(cd "$1" && pwd); this=$(cd "$2" && pwd)
out=${3:-$(mktemp -d)}
mkdir -p "$out"
out=$(cd "$out" && pwd)
files=${4:-mpp_sampler mpp_sampler_hbm mpp_deep mpp_hot}
pkg=mpp_cnn_rs_object_detection_amd
flags() { (cd "$this/$pkg" && python3 -c 'import build, sys; print(" ".join(build.FLAGS + build.EXTRA.get(sys.argv[1], [])))' $1.hip); }
hipcc=${HIPCC:-/opt/rocm/bin/hipcc}
compile() {   # tree, directory of the .s files
  mkdir -p "$2"
  for f in $files; do
    ( cd "$1/$pkg/csrc" && $hipcc $(flags $f) --cuda-device-only -S $f.hip -o "$2/$f.s" 2> "$2/$f.log" ) &
  done
  wait
  for f in $files; do [ -s "$2/$f.s" ] || { echo "compiling $f.hip of $1 failed:" >&2; cat "$2/$f.log" >&2; exit 2; }; done
}
[ -n "$3" ] && [ -s "$out/parent/${files%% *}.s" ] || compile "$parent" "$out/parent"
compile "$this" "$out/this"
python3 - "$out" $files <<'EOF'
import os, re, subprocess, sys, tempfile
out, files = sys.argv[1], sys.argv[2:]
FIELDS = ["vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"]

def read(path):
    lines = [l for l in open(path) if "__hip_cuid" not in l]
    txt = "".join(lines)
    meta = {}
    for blk in re.split(r"\n\s+- \.agpr_count", txt)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = [int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in FIELDS]
    body, cur = {}, None                    # the lines of each kernel, from its label to its .Lfunc_end
    for l in lines:
        m = re.match(r"(\w+):", l)
        if m and m.group(1) in meta:
            cur = body.setdefault(m.group(1), [])
        if cur is not None:
            cur.append(l)
            if l.startswith(".Lfunc_end"):
                cur = None
    return lines, meta, body

def ndiff(a, b, tmp):
    if a == b:
        return 0
    pa, pb = os.path.join(tmp, "a"), os.path.join(tmp, "b")
    open(pa, "w").writelines(a); open(pb, "w").writelines(b)
    r = subprocess.run(["diff", pa, pb], capture_output=True, text=True)
    return sum(1 for l in r.stdout.splitlines() if l[:1] in "<>")

def short(n):                               # template arguments of a mangled instantiation, e.g. 8,0,0,2,0,1
    m = re.search(r"kernelI(.*?)EvP?", n) or re.search(r"kernelI(.*)", n)
    args = re.findall(r"L[bij](\d+)E", m.group(1)) if m else []
    base = re.search(r"(mpp_\w+?_kernel)", n)
    return (base.group(1) if base else n) + "<" + ",".join(args) + ">"

bad = 0
with tempfile.TemporaryDirectory() as tmp:
    for f in files:
        la, ma, ba = read(os.path.join(out, "parent", f + ".s"))
        lb, mb, bb = read(os.path.join(out, "this", f + ".s"))
        total = ndiff(la, lb, tmp)
        bad += total
        print("## %s.hip: %d kernels, %d differing lines in the file" % (f, len(ma), total))
        print("| kernel | differing lines | " + " | ".join(FIELDS) + " |")
        print("|---|---|" + "---|" * len(FIELDS))
        for n in sorted(set(ma) | set(mb), key=short):
            if n not in ma or n not in mb:
                print("| %s | only in %s |" % (short(n), "parent" if n in ma else "this tree") + " |" * len(FIELDS))
                bad += 1
                continue
            d = ndiff(ba.get(n, []), bb.get(n, []), tmp)
            cells = [str(x) if x == y else "%d -> %d" % (x, y) for x, y in zip(ma[n], mb[n])]
            if total == 0 and "-v" not in os.environ.get("CODEOBJ_DIFF", ""):
                continue                    # an identical file: one summary line below instead of its kernels
            print("| %s | %d | " % (short(n), d) + " | ".join(cells) + " |")
        if total == 0:
            print("| all %d | 0 | equal | equal | equal | equal | equal |" % len(ma))
        print()
sys.exit(1 if bad else 0)
EOF
