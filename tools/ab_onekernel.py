"""Interleaved A/B of builds of the trainer step (the sibling of ab_wave_quad.py
for arms that are compile-time macros): one worker process per arm, each with
its own library (HGX_LIB_PATH) and the same records and initial model; the
parent alternates single epochs between the workers, so every round times
every arm once, back to back, and only one worker trains at a time. Per-batch
device time is hgx_train_last_stats (HIP events around each chunk's step
launches). Diagnostic only.

  tools/build_variant.sh ok0_fx0 hgx_train.hip "-DHGX_TRAIN_ONEKERNEL=0 -DHGX_TRAIN_FIXMAGIC=0"
  tools/build_variant.sh ok1_fx0 hgx_train.hip "-DHGX_TRAIN_ONEKERNEL=2 -DHGX_TRAIN_FIXMAGIC=0"
  tools/build_variant.sh ok0_fx1 hgx_train.hip "-DHGX_TRAIN_ONEKERNEL=0 -DHGX_TRAIN_FIXMAGIC=2"
  python tools/ab_onekernel.py 128 [rounds=6]            d = 128, C3 HOBE records
  python tools/ab_onekernel.py 256 [rounds=6] [frac=0.02]  d = 256, the C4 HOBE slice

Arms: base (two step kernels and the per-chunk flag wait, the rounding
intrinsic: the step as it was), A (one kernel per paired / quad form, no
wait), B (the add-constant to_fix everywhere), AB (the library as built), and
at d = 128 AB4 (AB with train_wave_pair 4, while the library accepts the
value). AB_LIBS=NAME=PATH,... adds libraries, AB_ARMS=NAME:LIB:PAIR,... names
the arms (PAIR = train_wave_pair) and AB_COMPARE=ARM:REF,... the comparisons.
Round 0 (warm-up) is not counted. Rules: A stays if it is no
slower than base by more than 0.045 us per batch; B stays if it is not
slower; a train_wave_pair value becomes the default only if it is faster than
the current default in every round and its mean gain is at least three
standard deviations of the current default's runs. The logs of
profiles/r10/trainer_onekernel/ were taken while AB was A and B together."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(d, frac):
  from hypergraphembedding_amd import _hgx
  from hypergraphembedding_amd.synthetic import powerlaw_hypergraph, random_hypergraph
  ctx = _hgx.Context(0)
  if d == 128:  # C3: random 100k/50k graph, 2M of its HOBE records
    inc = random_hypergraph(seed=0)
    ctx.upload(inc)
    r = np.random.RandomState(4)
    ctx.alg_set(r.random_sample((inc.N, 10)), r.random_sample((inc.E, 10)))
    ctx.alg_run(20)
    m = ctx.sample_hobe(17, 5, 200)
    idx, tgt = ctx.records_get()
    sel = np.random.RandomState(1).permutation(m)[:2_000_000]
    ctx.records_set(np.ascontiguousarray(idx[sel]), np.ascontiguousarray(tgt[sel]))
    n = len(sel)
  else:  # C4: power-law 10M/5M, a seeded row slice, full-size tables
    inc = powerlaw_hypergraph(seed=0)
    ctx.upload(inc)
    r = np.random.RandomState(1)
    ctx.alg_set(r.random_sample((inc.N, 10)).astype(np.float32),
                r.random_sample((inc.E, 10)).astype(np.float32))
    ctx.alg_run(20)
    rq = np.random.RandomState(2)
    nq = np.where(rq.random_sample(inc.N) < frac, 200, 0).astype(np.int32)
    eq = np.where(rq.random_sample(inc.E) < frac, 200, 0).astype(np.int32)
    n = ctx.sample_hobe(4000, 5, 200, node_q=nq, edge_q=eq)
  try:
    ctx.set_tuning("train_wave_pair", 4)
    has4 = True
  except Exception:
    has4 = False
  ctx.set_tuning("train_wave_pair", -1)
  print(json.dumps({"ready": True, "records": int(n), "has4": has4}), flush=True)
  for line in sys.stdin:
    pair = int(line)
    ctx.set_tuning("train_wave_pair", pair)
    ctx.model_init(d, inc.N + 2, inc.E + 2, seed=11)
    ctx.train(batch=256, max_epochs=1, loss=_hgx.LOSS_MSE, act=_hgx.ACT_RELU,
              min_delta=-1e30, shuffle_seed=2)
    ms, rec, bat = ctx.train_stats()
    print(json.dumps({"per_batch_us": ms * 1e3 / bat,
                      "geometry": ctx.train_step_geometry(),
                      "multi": ctx.train_multi_pending(),
                      "loss": float(ctx.train_loss_sum() / rec)}), flush=True)
  ctx.close()


def main():
  d = int(sys.argv[1]) if len(sys.argv) > 1 else 128
  rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 6
  frac = sys.argv[3] if len(sys.argv) > 3 else "0.02"
  ab = os.path.join(ROOT, "tools", "_ab")
  libs = {"base": os.path.join(ab, "ok0_fx0.so"), "A": os.path.join(ab, "ok1_fx0.so"),
          "B": os.path.join(ab, "ok0_fx1.so"), "AB": None}
  # further builds: AB_LIBS=NAME=PATH,...
  for t in filter(None, os.environ.get("AB_LIBS", "").split(",")):
    libs[t.split("=")[0]] = os.path.join(ROOT, t.split("=")[1])
  if os.environ.get("AB_ARMS"):  # only the libraries the named arms use (and AB)
    used = {t.split(":")[1] for t in os.environ["AB_ARMS"].split(",")} | {"AB"}
    libs = {k: v for k, v in libs.items() if k in used}
  procs = {}
  for name, path in libs.items():
    env = dict(os.environ)
    env.pop("HGX_LIB_PATH", None)
    if path:
      env["HGX_LIB_PATH"] = path
    procs[name] = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker",
                                    str(d), frac], stdin=subprocess.PIPE,
                                   stdout=subprocess.PIPE, text=True, env=env)
  ready = {name: json.loads(p.stdout.readline()) for name, p in procs.items()}
  print(json.dumps({"d": d, "ready": ready}), flush=True)
  arms = [(name, name, -1) for name in libs]
  if d == 128 and ready["AB"]["has4"]:
    arms.append(("AB4", "AB", 4))
  if os.environ.get("AB_ARMS"):  # NAME:LIB:PAIR,... (LIB one of the names above)
    arms = [(a, b, int(c)) for a, b, c in
            (t.split(":") for t in os.environ["AB_ARMS"].split(","))]
  res = {arm: [] for arm, _, _ in arms}
  for rnd in range(rounds + 1):
    for arm, proc, pair in arms:
      p = procs[proc]
      p.stdin.write(f"{pair}\n")
      p.stdin.flush()
      line = p.stdout.readline()
      if not line:  # the worker died: stop here, start nothing more
        print(json.dumps({"round": rnd, "arm": arm, "error": "worker exited"}), flush=True)
        for q in procs.values():
          q.stdin.close()
        sys.exit(1)
      o = json.loads(line)
      if rnd > 0:
        res[arm].append(o["per_batch_us"])
      o["per_batch_us"] = round(o["per_batch_us"], 4)
      print(json.dumps({"round": rnd, "arm": arm, **o}), flush=True)
  for p in procs.values():
    p.stdin.close()
  for p in procs.values():
    p.wait()

  def stat(v):
    return {"mean": round(float(v.mean()), 4), "std": round(float(v.std(ddof=1)), 4),
            "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}

  r = {k: np.array(v) for k, v in res.items()}
  out = {"d": d, "us": {k: stat(v) for k, v in r.items()}}
  pairs = [("A", "base"), ("B", "base"), ("AB", "base"), ("AB4", "AB")]
  if os.environ.get("AB_COMPARE"):  # ARM:REF,...
    pairs = [tuple(t.split(":")) for t in os.environ["AB_COMPARE"].split(",")]
  for arm, ref in pairs:
    if arm not in r or ref not in r:
      continue
    gain = r[ref] - r[arm]
    out[f"{arm}_vs_{ref}"] = {
        "gain_us": {"mean": round(float(gain.mean()), 4), "min": round(float(gain.min()), 4)},
        "faster_every_round": bool((gain > 0).all()),
        "gain_over_3_sigma": bool(gain.mean() >= 3 * r[ref].std(ddof=1)),
    }
  print(json.dumps(out), flush=True)


if __name__ == "__main__":
  if len(sys.argv) > 1 and sys.argv[1] == "--worker":
    worker(int(sys.argv[2]), float(sys.argv[3]))
  else:
    main()
