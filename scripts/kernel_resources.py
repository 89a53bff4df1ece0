"""Compiler resource report of the MFMA kernels and the NMS kernels (hipcc -Rpass-analysis=kernel-resource-usage, gfx950, no GPU
needed): file | kernel | VGPRs | AGPRs | scratch B/lane | VGPR spills | occupancy waves/SIMD -> stdout.

    python scripts/kernel_resources.py [--isa] [--csrc DIR] [file.hip ...]

--isa adds SGPRs, the LDS bytes per block and the number of instructions of the kernel's gfx950 assembly (hipcc -S, device only: the lines
between the kernel's label and its s_endpgm that are neither labels, directives nor comments).  --csrc DIR compiles the files of another
source tree's csrc (a checkout of an earlier commit) with this tree's flags, for an old-against-new table."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tiny-faces-pytorch_amd"))
from build import COMMON, CSRC, EXACT, HIPCC          # the shipped build's compiler and flags: -ffp-contract=off for the files in EXACT
ARGS = sys.argv[1:]
ISA = "--isa" in ARGS
if ISA:
    ARGS.remove("--isa")
if "--csrc" in ARGS:
    CSRC = os.path.abspath(ARGS[ARGS.index("--csrc") + 1])
    del ARGS[ARGS.index("--csrc"):ARGS.index("--csrc") + 2]
FILES = ARGS or ["conv_dma_bf16.hip", "conv_dma_f16.hip", "conv_dma.hip", "conv3x3h.hip", "wgrad_group.hip", "wgrad_dma.hip", "wgrad3x3.hip", "wgrad.hip", "conv.hip", "stem_conv.hip", "nms.hip"]


def demangle(name):
    name = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
    return name.replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")


def instruction_counts(f, flags):
    """{mangled kernel name: instructions} from the device assembly of csrc/f."""
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([HIPCC] + COMMON + flags + ["-S", "--cuda-device-only", os.path.join(CSRC, f), "-o", out], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        asm = open(out).read()
    counts = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\s*s_endpgm", asm, re.S | re.M):
        body = [l.strip() for l in m.group(2).splitlines()]
        counts[m.group(1)] = 1 + sum(1 for l in body if l and not l.startswith((";", ".", "//")) and not l.endswith(":"))
    return counts


print("# compiler resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) of the MFMA kernels and the NMS kernels")
print("# file | kernel | VGPRs | AGPRs | scratch B/lane | VGPR spills | occupancy waves/SIMD" + (" | SGPRs | LDS B/block | instructions" if ISA else ""))
for f in FILES:
    flags = ["-ffp-contract=off"] if f in EXACT else []
    r = subprocess.run([HIPCC] + COMMON + flags + ["-c", os.path.join(CSRC, f), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True)
    icount = instruction_counts(f, flags) if ISA else {}
    cur = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs Spill|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2)
        if k == "Function Name":
            cur = {"name": v}
        else:
            cur[k] = v
        if k == ("LDS Size [bytes/block]" if ISA else "VGPRs Spill"):
            if all(x in cur for x in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "Occupancy [waves/SIMD]")):
                row = f"{f} | {demangle(cur['name'])} | {cur['VGPRs']} | {cur['AGPRs']} | {cur['ScratchSize [bytes/lane]']} | {cur['VGPRs Spill']} | {cur['Occupancy [waves/SIMD]']}"
                if ISA:
                    row += f" | {cur.get('TotalSGPRs', '?')} | {cur['LDS Size [bytes/block]']} | {icount.get(cur['name'], '?')}"
                print(row)
                cur = {}
