#!/bin/bash
# registers / scratch of every instantiation of the chain kernels in a built object:
#   bash profiles/tools/kernel_regs.sh [path/to/mpp_sampler.o | path/to/mpp_deep.o | path/to/mpp_hot.o]
# mpp_chain_kernel: WAVES,LPW,DIAG,OCC,SM,FAST; mpp_deep_kernel: WAVES,DIAG,OCC,EXT[,TAB[,QUE[,NCH]]]; mpp_hot_kernel: WAVES,OCC
# or of the kernels of any object whose mangled names contain a word:
#   bash profiles/tools/kernel_regs.sh path/to/mpp_recombine.o k_recombine
obj=${1:-mpp_cnn_rs_object_detection_amd/csrc/mpp_sampler.o}
export KERNEL_REGS_WORD=$2
tmp=$(mktemp -d)
B=/opt/rocm/lib/llvm/bin
$B/llvm-objcopy -O binary --only-section=.hip_fatbin $obj $tmp/fat.bin
$B/clang-offload-bundler --type=o --targets=hipv4-amdgcn-amd-amdhsa--gfx950 --input=$tmp/fat.bin --output=$tmp/dev.co --unbundle
$B/llvm-readelf --notes $tmp/dev.co | python3 -c '
import os, re, sys
word = os.environ.get("KERNEL_REGS_WORD", "")
txt = sys.stdin.read()
for blk in re.split(r"\n\s+- \.agpr_count", txt)[1:]:
    name = re.search(r"\.name:\s+(\S+)", blk)
    if not name: continue
    n = name.group(1)
    g = lambda k: re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)
    if word:
        if word not in n: continue
        label = n
    elif "mpp_chain_kernel" in n:
        targs = re.search(r"ILi(\d+)ELi(\d+)ELb(\d)ELi(\d+)ELb(\d)ELb(\d)E", n)
        label = "WAVES,LPW,DIAG,OCC,SM,FAST = " + (",".join(targs.groups()) if targs else n)
    elif "mpp_deep_kernel" in n:
        targs = re.search(r"ILi(\d+)ELb(\d)ELi(\d+)ELb(\d)E(?:Lb(\d)E)?(?:Lb(\d)E)?(?:Li(\d+)E)?", n)
        label = "deep WAVES,DIAG,OCC,EXT,TAB[,QUE[,NCH]] = " + (",".join(v for v in targs.groups() if v is not None) if targs else n)
    elif "mpp_hot_kernel" in n:
        targs = re.search(r"ILi(\d+)ELi(\d+)E", n)
        label = "hot WAVES,OCC = " + (",".join(targs.groups()) if targs else n)
    else:
        continue
    print(label, " vgpr", g("vgpr_count"), "spill", g("vgpr_spill_count"), "sgpr", g("sgpr_count"), "sgpr_spill", g("sgpr_spill_count"), "scratch", g("private_segment_fixed_size"))
' | sort
rm -rf $tmp
