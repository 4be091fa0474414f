#!/usr/bin/env python3
"""Count the dependent memory rounds of the convolution kernels in a gfx950 listing.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S conv_igemm.hip -o conv_igemm.s \
          -Rpass-analysis=kernel-resource-usage 2> conv_igemm.res
    python tools/conv_rounds.py conv_igemm.s conv_igemm.res [name filter ...]

Per kernel whose demangled name contains one of the filters (default: the ring, tile and weight-gradient ring kernels):
  head    scalar waits (s_waitcnt with lgkmcnt) in front of the first vector-memory load, in listing order (the early-exit
          test of a workgroup without work sits in front of it and is counted with it);
  loads   vector loads that can run after an output store of the vector path (a 4-element store of a lane): reachable from it in
          the control-flow graph.  "Epilogue" = behind the last MFMA of the listing (normalise-on-load stores inside the main loop
          are not epilogue stores).  Single-element loads are counted apart: the element-by-element form of the segmentation head
          (ragged cout, NCHW) keeps its few loads between its stores, and the listing cannot show that a launch takes one form only;
  waits   s_waitcnt with a vmcnt between such a store and any later epilogue store (partial rows included), listed by their counts:
          vmcnt(k) lets the k youngest operations stay in flight, so only a count below the number of stores issued before it
          waits for a store's acknowledgement;
  VGPRs, SGPRs, scratch, occupancy from the resource remarks.
Counting only: nothing here judges the listing."""
import re
import shutil
import subprocess
import sys

LOAD = re.compile(r"^\s+(global_load|buffer_load|flat_load|scratch_load)")
STORE = re.compile(r"^\s+(global_store|buffer_store|flat_store)")
WIDE = re.compile(r"_store_dwordx[24]\b")      # the vector path's output stores (4 elements a lane); partial rows and the ragged path store single elements
WIDEL = re.compile(r"_load_dwordx[234]\b")     # vector-path loads; the head's element-by-element form loads single elements between its stores
WAIT = re.compile(r"^\s+s_waitcnt\b(.*)")
BRANCH = re.compile(r"^\s+(s_cbranch_\w+|s_branch)\s+(\S+)")
LABEL = re.compile(r"^(\.LBB\S+):")
DEFAULT = ("conv_ring_kernel", "conv_igemm_kernel", "conv_wgrad_ring_kernel")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path):
    """{mangled name: list of instruction / label lines}"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].rstrip()
        if LABEL.match(s) or (s[:1] in "\t " and s.strip() and not s.strip().startswith(".")):
            cur.append(s)
    return out


def resources(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif cur is not None:
            cur[m.group(1).split(" ")[0]] = m.group(2)
    return out


def successors(lines):
    label_at = {LABEL.match(s).group(1): i for i, s in enumerate(lines) if LABEL.match(s)}
    succ = []
    for i, s in enumerate(lines):
        nxt = [i + 1] if i + 1 < len(lines) else []
        m = BRANCH.match(s)
        if m:
            tgt = label_at.get(m.group(2))
            nxt = ([tgt] if tgt is not None else []) + ([] if m.group(1) == "s_branch" else nxt)
        elif s.strip().startswith("s_endpgm"):
            nxt = []
        succ.append(nxt)
    return succ


def reach(starts, succ):
    """instructions reachable from (strictly after) any of starts"""
    seen, todo = set(), [t for s in starts for t in succ[s]]
    while todo:
        i = todo.pop()
        if i in seen:
            continue
        seen.add(i)
        todo.extend(succ[i])
    return seen


def analyse(lines):
    first_load = next((i for i, s in enumerate(lines) if LOAD.match(s)), len(lines))
    head = sum(1 for s in lines[:first_load] if WAIT.match(s) and "lgkmcnt" in s)
    mfma = [i for i, s in enumerate(lines) if "v_mfma" in s]
    tail = mfma[-1] if mfma else 0
    succ = successors(lines)
    pred = [[] for _ in lines]
    for i, ns in enumerate(succ):
        for t in ns:
            pred[t].append(i)
    stores = [i for i, s in enumerate(lines) if i > tail and STORE.match(s)]
    wide = [i for i in stores if WIDE.search(lines[i])]
    after = reach(wide, succ)
    before = reach(stores, pred)
    loads = sum(1 for i in after if i > tail and LOAD.match(lines[i]) and WIDEL.search(lines[i]))
    single = sum(1 for i in after if i > tail and LOAD.match(lines[i]) and not WIDEL.search(lines[i]))
    waits = []
    for i in sorted(after & before):
        m = WAIT.match(lines[i])
        if m and "vmcnt" in m.group(1):
            waits.append(re.search(r"vmcnt\((\d+)\)", m.group(1)).group(1))
    return head, loads, single, waits, len(stores)


def main():
    asm, res, *filters = sys.argv[1:]
    filters = filters or DEFAULT
    ks, rs = kernels(asm), resources(res)
    names = demangle(list(ks))
    for k in sorted(ks, key=lambda k: names[k]):
        if not any(f in names[k] or f in k for f in filters):
            continue
        head, loads, single, waits, nst = analyse(ks[k])
        r = rs.get(k, {})
        short = re.sub(r"\(.*", "", names[k]).replace("(anonymous namespace)::", "").replace("void ", "")
        print(f"{short}: head {head}  loads-after-store {loads} (+{single} single-element)  vmcnt-between-stores [{' '.join(waits)}] of {nst} stores  "
              f"VGPRs {r.get('VGPRs')} SGPRs {r.get('TotalSGPRs')} scratch {r.get('ScratchSize')} occupancy {r.get('Occupancy')}")


if __name__ == "__main__":
    main()
