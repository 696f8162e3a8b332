"""aggregate env-steps/s of S independent ICRL runs (BASELINE configs[1] each) sharing one MI355X inside the launches; --cpg: of S cpg runs
(cpg_bench below); --gail: of S gail runs (gail_bench below)."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from icrl_amd import seed_batch as SB



def cpg_config(which, seed):
    """configs4: BASELINE configs[4]'s 512-env shard with its frozen constraint net (bench.config_cpg); hc64: HCWithPos x 64 envs against the
    ground-truth wall cost (an AnalyticCost: the batched analytic-cost kernels), default cpg flags otherwise."""
    import types
    from icrl_amd.cpg import build_parser
    if which == "configs4":
        return bench.config_cpg(seed, 0, 1)
    cfg = vars(build_parser().parse_args(["cpg", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "64", "-s", str(seed), "-v", "0", "-t", "2e6"]))
    cfg.update(rank=0, world_size=1, save_dir=None)
    return types.SimpleNamespace(**cfg)


def cpg_bench(argv):
    """python tools/seed_batch_bench.py --cpg [--solo] [--workloads configs4,hc64] [--seeds 1,4,8,32] [--steps K] [--warmup W] [--reps R] [--out FILE]
    One JSON line per (workload, S): aggregate env-steps/s of S cpg runs advancing in lock-step (CpgSeedBatch), R timed learn() calls of K
    rollouts + updates each after W warm-up rollouts (median, min, max).  --solo: ONE run through cpg.setup + PPOLagrangian.learn, timed the
    same way — the sequential aggregate of S seeds is that rate, since the runs then go one after another."""
    import argparse, json
    from icrl_amd import cpg as C
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpg", action="store_true"); ap.add_argument("--solo", action="store_true")
    ap.add_argument("--workloads", default="configs4,hc64"); ap.add_argument("--seeds", default="1,4,8,32")
    ap.add_argument("--steps", type=int, default=2); ap.add_argument("--warmup", type=int, default=1); ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    for which in a.workloads.split(","):
        for S in ([1] if a.solo else [int(x) for x in a.seeds.split(",")]):
            cfgs = [cpg_config(which, seed) for seed in range(S)]
            per = cfgs[0].num_threads * cfgs[0].n_steps
            if a.solo:
                model, cb, learn_cost, _ = C.setup(cfgs[0], log=None)
                learn = lambda k: model.learn(total_timesteps=k * per, cost_function=learn_cost, callback=cb)
            else:
                sb = SB.CpgSeedBatch(cfgs)
                cbs = [st["callback"] for st in sb.states]
                learn = lambda k: sb._learn(k * per, callbacks=cbs, prefetch_across_end=False)
            learn(a.warmup)
            rates = []
            for _ in range(a.reps):
                torch.cuda.synchronize(); t0 = time.time()
                learn(a.steps)
                torch.cuda.synchronize(); rates.append(S * a.steps * per / (time.time() - t0))
            rates.sort()
            rec = dict(workload=which, driver="solo" if a.solo else "batch", S=S, envs=cfgs[0].num_threads, n_steps=cfgs[0].n_steps, steps=a.steps, warmup=a.warmup,
                       reps=a.reps, env_steps_per_s_median=round(rates[len(rates) // 2], 1), env_steps_per_s_min=round(rates[0], 1),
                       env_steps_per_s_max=round(rates[-1], 1))
            print(json.dumps(rec), flush=True)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, "a") as fh:
                    fh.write(json.dumps(rec) + "\n")
            if a.solo:
                del model, cb
            else:
                del sb, cbs
            del learn
            torch.cuda.empty_cache()


def gail_config(seed):
    """HCWithPos x 64 envs with README's gail flags (-dl 30 -dlr 0.003 -lc -tk 0.01, 10 expert rollouts), default gail flags otherwise."""
    import types
    from icrl_amd.gail import build_parser
    cfg = vars(build_parser().parse_args(["gail", "-tei", "HCWithPos-v0", "-eei", "HCWithPosTest-v0", "-nt", "64", "-er", "10", "-tk", "0.01", "-dl", "30",
                                          "-dlr", "0.003", "-lc", "-s", str(seed), "-v", "0", "-t", "2e6"]))
    cfg.update(rank=0, world_size=1, save_dir=None)
    return types.SimpleNamespace(**cfg)


def gail_bench(argv):
    """python tools/seed_batch_bench.py --gail [--solo] [--seeds 1,4,8,32] [--steps K] [--warmup W] [--reps R] [--out FILE]
    One JSON line per S: aggregate env-steps/s of S gail runs advancing in lock-step (GailSeedBatch: rollouts, evaluations, the
    discriminator's rollout-end work and updates of all runs in one launch sequence each), R timed learn() calls of K rollout + update rounds
    each after W warm-up rounds (median, min, max).  --solo: ONE run through gail.setup + PPO.learn, timed the same way — the sequential
    aggregate of S seeds is that rate.  Without --solo the solo run is timed before and after every batched S in the same call (the two
    versions alternated; `solo_before` / `solo_after` in the record).  PHASES=1: the host-clock share of the phases of one more round."""
    import argparse, json
    from icrl_amd import gail as G
    ap = argparse.ArgumentParser()
    ap.add_argument("--gail", action="store_true"); ap.add_argument("--solo", action="store_true")
    ap.add_argument("--seeds", default="1,4,8,32"); ap.add_argument("--steps", type=int, default=5); ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3); ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    per = gail_config(0).num_threads * gail_config(0).n_steps

    def timed(learn, S):
        learn(a.warmup)
        rates = []
        for _ in range(a.reps):
            torch.cuda.synchronize(); t0 = time.time()
            learn(a.steps)
            torch.cuda.synchronize(); rates.append(S * a.steps * per / (time.time() - t0))
        rates.sort()
        return dict(env_steps_per_s_median=round(rates[len(rates) // 2], 1), env_steps_per_s_min=round(rates[0], 1), env_steps_per_s_max=round(rates[-1], 1))

    def solo():
        model, cb, disc, _ = G.setup(gail_config(0), log=None)
        r = timed(lambda k: model.learn(total_timesteps=k * per, callback=cb), 1)
        del model, cb, disc
        torch.cuda.empty_cache()
        return r

    def emit(rec):
        print(json.dumps(rec), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
    common = dict(workload="gail_hc64", envs=gail_config(0).num_threads, n_steps=gail_config(0).n_steps, steps=a.steps, warmup=a.warmup, reps=a.reps)
    if a.solo:
        emit(dict(common, driver="solo", S=1, **solo()))
        return
    for S in [int(x) for x in a.seeds.split(",")]:
        before = solo()
        sb = SB.GailSeedBatch([gail_config(seed) for seed in range(S)])
        cbs = [st["callback"] for st in sb.states]
        learn = lambda k: sb._learn(k * per, callbacks=cbs, prefetch=False)
        rec = dict(common, driver="batch", S=S, **timed(learn, S))
        if os.environ.get("PHASES"):      # where one more lock-step round goes (host clock, synchronised at the phase boundaries)
            t = {}
            names = ("_launch_rollouts", "_evaluations", "_gail_rollout_ends", "_launch_trains")
            orig = {k: getattr(SB.SeedBatch, k) for k in names}

            def wrap(name, fn):
                def w(self, *args, **kw):
                    torch.cuda.synchronize(); t0 = time.time()
                    r = fn(self, *args, **kw)
                    torch.cuda.synchronize(); t[name] = t.get(name, 0.0) + time.time() - t0
                    return r
                return w
            for k, fn in orig.items():
                setattr(SB.SeedBatch, k, wrap(k, fn))
            torch.cuda.synchronize(); t0 = time.time()
            learn(1)
            torch.cuda.synchronize(); tot = time.time() - t0
            for k, fn in orig.items():
                setattr(SB.SeedBatch, k, fn)
            rec["phases_ms"] = dict({k: round(1e3 * v, 2) for k, v in t.items()}, round_total=round(1e3 * tot, 2))
        del sb, cbs, learn
        torch.cuda.empty_cache()
        after = solo()
        rec.update(solo_before=before["env_steps_per_s_median"], solo_after=after["env_steps_per_s_median"])
        emit(rec)


if "--gail" in sys.argv[1:]:
    gail_bench(sys.argv[1:])
    sys.exit(0)

if "--cpg" in sys.argv[1:]:
    cpg_bench(sys.argv[1:])
    sys.exit(0)

for S in [int(x) for x in os.environ.get("SEEDS", "1,8,32,64").split(",")]:
    sb = SB.SeedBatch([bench.config2(4 + int(os.environ.get('ITERS', '2')), seed, 0, 1) for seed in range(S)])
    sb.run(0, 1)
    steps0 = sum(st["timesteps"] for st in sb.states)
    n_it = int(os.environ.get("ITERS", "2"))
    _, dt = sb.run(1, n_it)
    steps = sum(st["timesteps"] for st in sb.states) - steps0
    print(f"S={S:3d}: {n_it} iterations of every run in {dt:6.2f} s -> {steps / dt / 1e6:7.3f} M env-steps/s aggregate ({steps / dt / S / 1e3:7.1f} k per run)", flush=True)
    if os.environ.get("PHASES"):       # where one lock-step iteration goes (host clock, synchronised at the phase boundaries)
        import icrl_amd.seed_batch as M
        t = {}
        orig = {k: getattr(M.SeedBatch, k) for k in ("_learn", "_episodes", "_launch_cn_trains")}
        def timed(name, fn):
            def w(self, *a, **k):
                torch.cuda.synchronize(); t0 = time.time()
                r = fn(self, *a, **k)
                torch.cuda.synchronize(); t[name] = t.get(name, 0.0) + time.time() - t0
                return r
            return w
        for k, fn in orig.items():
            setattr(M.SeedBatch, k, timed(k, fn))
        t0 = time.time(); sb.run(3, 1); tot = time.time() - t0
        for k, fn in orig.items():
            setattr(M.SeedBatch, k, fn)
        print("      one iteration %.1f ms: " % (1e3 * tot) + ", ".join(f"{k} {1e3 * v:.1f} ms" for k, v in t.items()), flush=True)
    del sb
    torch.cuda.empty_cache()
