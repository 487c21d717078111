"""Static instruction census of one kernel in a gfx950 assembly listing
(hipcc -S --cuda-device-only): the instructions between the kernel's entry,
its record-word loads (the third global_load_dword), its workgroup barriers
and s_endpgm, by class. Static: every role program and every rarely taken
branch of a segment is counted once, so a segment's count is an upper bound
of what one wave executes there; differences between two builds of the same
source structure are the instructions a change removed. Diagnostic only.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude \
      -mllvm -amdgpu-kernarg-preload-count=12 --cuda-device-only -S \
      hypergraphembedding_amd/csrc/hgx_train.hip -o train.s
  python tools/step_census.py train.s train_step_qILi2ELi5ELi2ELb0ELi1E"""
import re
import sys

TRANS = ("v_rcp", "v_rsq", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")
MEM = ("global_", "flat_", "buffer_", "scratch_", "ds_", "s_load", "s_buffer_load")


def classify(op):
  if op.startswith(MEM):
    return "memory"
  if op.startswith("s_waitcnt"):
    return "waitcnt"
  if op.startswith(("s_cbranch", "s_branch", "s_barrier", "s_endpgm", "s_nop", "s_setpc")):
    return "control"
  if op.startswith("s_"):
    return "scalar"
  if "_f64" in op:
    return "f64"
  if op.startswith(TRANS):
    return "transcendental"
  if op.startswith("v_"):
    return "valu"
  return "other"


def main():
  path, sym = sys.argv[1], sys.argv[2]
  lines = open(path).read().split("\n")
  start = next(i for i, l in enumerate(lines)  # the label line "NAME: ; @NAME"
               if l.startswith("_Z") and ":" in l and sym in l.split(":")[0])
  segs, cur, loads, names = [], {}, 0, ["entry to record-word loads", "to barrier 1",
                                       "to barrier 2", "to s_endpgm"]
  divs = []
  ndiv = 0
  for l in lines[start + 1:]:
    m = re.match(r"\t([a-z_0-9]+)", l)
    if not m:
      if l.startswith(".Lfunc_end"):
        break
      continue
    op = m.group(1)
    if op.startswith("."):
      continue
    cur[classify(op)] = cur.get(classify(op), 0) + 1
    ndiv += op.startswith("v_div_scale")
    cut = False
    if op == "global_load_dword" and len(segs) == 0:
      loads += 1
      cut = loads == 3
    cut |= op == "s_barrier"
    if cut:
      segs.append(cur)
      divs.append(ndiv)
      cur, ndiv = {}, 0
  segs.append(cur)
  divs.append(ndiv)
  keys = ["valu", "transcendental", "f64", "scalar", "memory", "waitcnt", "control"]
  print("%-28s" % "segment" + "".join("%9s" % k[:8] for k in keys) + "    total  v_div_scale")
  tot = {k: 0 for k in keys}
  for name, s, dv in zip(names, segs, divs):
    print("%-28s" % name + "".join("%9d" % s.get(k, 0) for k in keys) +
          "%9d%9d" % (sum(s.values()), dv))
    for k in keys:
      tot[k] += s.get(k, 0)
  print("%-28s" % "kernel" + "".join("%9d" % tot[k] for k in keys) +
        "%9d%9d" % (sum(tot.values()), sum(divs)))


if __name__ == "__main__":
  main()
