"""weights="fp8a" against weights="fp4a" in ONE process on ONE box, the two modes alternated (A B A B ...):

  head   the 6-block head at BitDance-14B width, 128 rows: one sampling run of n_steps + 1 evaluations as a hipGraph replay
         (us per evaluation) and the in-situ time of every GEMM launch of an eager run (bd_prof_*: the weights come from HBM)
  llm    a 12-layer slice of Qwen3-14B, 128 rows against ~1k cached tokens: the eager decode step (us per layer) and the same
         per-GEMM times
  image  one 1024-px image through BitDanceT2IPipeline on the synthetic 14B-64x model (bitdance_amd/synthetic.py), 50 sampling
         steps, guidance 7.5: warm-up 1 + 3 timed per mode

python tools/fp4a_compare.py head|llm|image [rounds] [--json out.json] [--tune k=v,k=v]      (--tune: head only, e.g. ada_group=1 = the
                                                                                             per-evaluation adaLN projection at 128 rows)

The five GEMMs that differ between the modes are head.ada / head.qkv / head.w1 and llm.qkv / llm.gu; everything else runs the same
code on the same bytes and shows the run-to-run spread of the session."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bitdance_amd import engine as E                       # noqa: E402
from bitdance_amd import synthetic as syn                   # noqa: E402

MODES = ("fp8a", "fp4a")


def per_gemm(prof: dict) -> dict:
    return {k: round(v["ms"] / v["count"] * 1e3, 2) for k, v in sorted(prof.items())}


def head(rounds: int, n: int = 50, tune: dict | None = None) -> list:
    from oracle import tiny_models as tm                    # (shape table + seeded random weights only)
    from oracle.true_dims import device_seeded_state
    dev = "cuda"
    cfgd = dict(ch_target=32, ch_cond=5120, ch_latent=5120, depth_latent=6, depth_adanln=2)
    sd = device_seeded_state(tm.head_shapes(cfgd), 101, dev)
    hw = {m: E.HeadWeights.from_state_dict(sd, dev, weights=m) for m in MODES}
    del sd
    g = torch.Generator(device=dev).manual_seed(7)
    cond = torch.randn(2, 64, 5120, device=dev, generator=g)
    noise = torch.randn(1, n + 1, 1, 64, 32, device=dev, generator=g)
    eng = {}
    for m in MODES:
        e = E.Engine(hw[m], None, None, num_images=1, branches=2, device=dev, max_tokens=64, parallel_num=64, tune=dict(tune or {}))
        e.set_schedule(n, 7.5, 1)
        e.load_noise(noise)
        e.reset([0, 0])
        e.set_cond(cond)
        e.head_sample()
        torch.cuda.synchronize()
        e.capture(0)
        eng[m] = e
    print("# launch configurations (split-K, waves + 16 ring + 256 (kparts - 1)): " +
          "; ".join(f"{m}: " + ", ".join(f"{k} {eng[m].gemm_config('head.' + k)}" for k in ("ada", "qkv", "wo", "w1", "w2")) for m in MODES), flush=True)
    out = []
    for r in range(rounds):
        for m in MODES:
            e = eng[m]
            ts = []
            for _ in range(3):
                e.reset([0, 0])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e.launch(0)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)

            def eager():
                e.reset([0, 0])
                e.head_sample()
            pg = per_gemm(e.profile_gemms(eager))
            rec = {"what": "head", "round": r, "mode": m, "us_per_eval_graph": round(min(ts) / (n + 1) * 1e6, 1),
                   "us_per_eval_graph_median": round(sorted(ts)[1] / (n + 1) * 1e6, 1), "gemm_us": pg}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def llm(rounds: int, layers: int = 12, past: int = 1024) -> list:
    dev = "cuda"
    cfg = dict(syn.QWEN3_14B)
    cfg["num_hidden_layers"] = layers
    cfg["vocab_size"] = 1024
    sd = syn.random_llm_state(cfg, dev)
    lw = {m: E.LlmWeights.from_state_dict(sd, cfg, dev, keep_for_prefill=False, weights=m) for m in MODES}
    del sd
    x = torch.randn(128, cfg["hidden_size"], device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    eng = {m: E.Engine(None, None, lw[m], num_images=1, branches=2, device=dev, max_tokens=64, max_kv=past + 256) for m in MODES}
    for e in eng.values():
        e.set_int("rt.emit_cond", 0)
    print("# launch configurations: " + "; ".join(f"{m}: " + ", ".join(f"{k} {eng[m].gemm_config('llm.' + k)}" for k in ("qkv", "o", "gu", "down"))
                                                   for m in MODES), flush=True)
    st = torch.cuda.current_stream()
    out = []
    for r in range(rounds):
        for m in MODES:
            e = eng[m]

            def step():
                e.reset([past, past - 5])
                e.residual()[:128].copy_(x)
                e.llm_step()
            step()
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                e.reset([past, past - 5])
                e.residual()[:128].copy_(x)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                e.llm_step()
                e1.record(st)
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            rec = {"what": "llm", "round": r, "mode": m, "us_per_layer": round(min(ts) / layers * 1e3, 1),
                   "us_per_layer_median": round(sorted(ts)[2] / layers * 1e3, 1), "gemm_us": per_gemm(e.profile_gemms(step))}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def image(rounds: int) -> list:
    out = []
    pipes = {}
    kw = dict(guidance_scale=7.5, num_sampling_steps=50, max_length=64 * 64, num_images=1, image_size=[1024, 1024])
    for m in MODES:
        pipes[m] = syn.build_pipeline("14b-64x", "cuda", with_ae=True, weights=m)
        torch.manual_seed(0)
        pipes[m].gen_image("a red fox", "<|", **kw)        # warm-up: graphs captured
        torch.cuda.synchronize()
    for r in range(rounds):
        for m in MODES:
            ts = []
            for _ in range(3):
                torch.manual_seed(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                img = pipes[m].gen_image("a red fox", "<|", **kw)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            rec = {"what": "image", "round": r, "mode": m, "s_per_image": [round(t, 4) for t in ts], "img_per_s_best": round(1 / min(ts), 4),
                   "img_per_s_median": round(1 / sorted(ts)[1], 4), "finite": bool(torch.isfinite(img).all())}
            print(json.dumps(rec), flush=True)
            out.append(rec)
    return out


def main():
    args = list(sys.argv[1:])
    path = None
    if "--json" in args:
        i = args.index("--json")
        path = args[i + 1]
        del args[i:i + 2]
    tune = None
    if "--tune" in args:
        i = args.index("--tune")
        tune = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in args[i + 1].split(",") if kv}
        del args[i:i + 2]
    what = args[0] if args else "head"
    rounds = int(args[1]) if len(args) > 1 else 2
    with torch.cuda.stream(torch.cuda.Stream()):
        recs = head(rounds, tune=tune) if what == "head" else {"llm": llm, "image": image}[what](rounds)
    if path:
        with open(path, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
