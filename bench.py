#!/usr/bin/env python3
"""bench.py - ProtNote train step (fwd + bwd + clip + Adam) on MI355X, BASELINE.json configs[2]/[3].

    python bench.py --gpus 1 --steps 3 --warmup 1
    python bench.py --gpus 8 --steps 3 --warmup 1            # no torchrun env: re-executes itself under
                                                              # torch.distributed.run with 8 ranks (RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W
    python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR   # also writes the last timed step's results as
                                                                        # DIR/*.npy (float32; see dump_outputs)

One "step" = one full optimisation step of the hot path on one batch of synthetic input per GPU: frozen
ProteInfer encoder forward (train-mode BN) -> W_p / W_l -> pair-grid MLP head with train-mode BatchNorm over
all B x N_L pairs -> BCE loss -> backward -> (N>1: RCCL all-reduce of the flat gradient) -> clip + Adam.
Per GPU: B=256 proteins, L=512, N_L=32102 labels (weak scaling).  Inputs are resident in HBM before the timed
region.  Rank 0's LAST stdout line is ONE compact JSON object (<= 4 kB: the contract keys, `roofline`, `cpu_baseline`,
a `modes` block of one-liners); the full record (`kernels`, `stages`, every sub-benchmark) goes to bench_detail.json
beside this script and to an earlier stdout line ({"bench_detail": ...}).

`roofline` describes the dominant kernel family (the 3072x3072 f32-MFMA GEMMs over the 8.2M-row pair grid):
achieved = 2*rows*h*h FLOP per launch / mean launch duration from hipEvents recorded on the launch stream
inside the timed region (pn_prof_begin/end); peak = 157.3 TFLOP/s (v_mfma_f32_32x32x2_f32, dense f32).
`cpu_baseline` times the CPU oracle's train step (a port of the reference algorithm, pinned to reference
golden vectors) on a bounded sample of the same workload, rank 0 at N=1 only.

Outside the headline timed region the same process also measures (each with its own `roofline`):
  `fast_mode`     the same train step on the opt-in bf16x3 arithmetic,
  `forward_only`  BASELINE configs[1]: eval forward, B=256 x L=512 x 32102 labels,
  `zero_shot`     BASELINE configs[4]: variable-length sequences (log-uniform 32..2048) in length buckets
                  {128..2048}, two descriptions per label ensembled, GO-sized label table then an EC-sized table
                  swapped in at run time on the same model object (sequences sharded over ranks at N>1),
  `comm`          (N>1) device time of every collective of the timed region.
"""
import argparse
import json
import math
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

KIND_NAMES = {
    0: "nt:plain", 10: "nt:bn_relu(z)", 20: "nt:pairsum_relu", 31: "nt:conv", 32: "nt:conv, f64 accumulation (trainable encoder)", 40: "nt:dz(elem)", 50: "nt:dz(rowg)",
    12: "nt:bn_relu(z)->rowdot", 22: "nt:pairsum_relu->rowdot", 3: "nt:plain->scale", 2: "nt:plain->rowdot",
    104: "tn:plain x conv tap (encoder wgrad)", 100: "tn:plain x plain", 101: "tn:plain x bn_relu", 102: "tn:plain x pairsum", 110: "tn:dz(elem) x plain", 111: "tn:dz(elem) x bn_relu",
    112: "tn:dz(elem) x pairsum", 121: "tn:dz(rowg) x bn_relu", 122: "tn:dz(rowg) x pairsum",
    900: "similarity backward: dP^ / dL^ contractions + normalisation backward (pn_similarity_bwd)",
}
_F32_KINDS = dict(KIND_NAMES)
KIND_NAMES.update({1000 + k: v + " [bf16x3]" for k, v in _F32_KINDS.items()})
# pn_set_backward_math(1): the hidden layers' backward pair-grid GEMMs on ONE bf16 product (f32 accumulation)
KIND_NAMES.update({1500 + k: v + " [bf16, one product]" for k, v in _F32_KINDS.items() if k < 500})
# forward_math = bf16 with the activation operand materialised as bf16 (fwd_bf16_h.hpp): all-DMA GEMM, kind 1700 + 10 * source
# (0 = a bf16 activation the previous layer's epilogue wrote, 1 = relu(bn(z)), 2 = pair sum) + epilogue (5 = stores bf16)
KIND_NAMES.update({1700 + 10 * a + e: f"nt:{an}->{en} [bf16, one product, operand materialised as bf16]"
                   for a, an in ((0, "h16"), (1, "bn_relu(z)"), (2, "pairsum_relu"))
                   for e, en in ((0, "store"), (2, "rowdot"), (5, "store h16"))})
# HBM-bound streaming stages (pn_prof kinds >= 2000; the library reports their ALGORITHMIC bytes, include/protnote_hip.h)
STAGE_NAMES = {
    2001: ("K2 conv1 from one-hots (k_ncl_to_nlc + 20-channel conv)", "4 B x (20 read + 1100 written) per residue"),
    2002: ("K6 masked mean-pool (k_pool)", "4 B x 1100 read per residue"),
    2003: ("K13/K14 loss + dlogits + TP/FN/FP (k_loss)", "4 B logit + 1 B target read, 4 B gradient written per pair "
                                                         "(the ABI takes i64 / f32 targets: 8 / 4 B actually read)"),
    2004: ("K16 clip + optimiser (k_sumsq + k_adam | k_sgd)", "Adam: 16 B read + 12 B written per parameter"),
    2005: ("dz in place (k_dz_apply)", "top layer: z read, dz written (8 B x h per row); inner: z, G read, dz written (12 B x h)"),
    2006: ("BatchNorm-backward statistics (k_bn_bwd_stats)", "top: z read (4 B x h per row); inner: z and G read (8 B x h)"),
    2007: ("layer-1 masked reduction (k_pair_mask_reduce_fused)", "G read once (4 B x h per row)"),
    2008: ("row-dot logits (k_rowdot_rows_reg)", "top pre-activation read (4 B x h per row), 4 B written"),
    2009: ("conv operand staging (k_conv_stage_act)", "activation read + staged image written"),
    2010: ("forward operand materialised as bf16 (k_make_h_bf16)", "2 B x h written per row; from a stored z also 4 B x h read "
                                                                  "(the pair-sum kind reads L2-resident tables)"),
}
# VALU-bound stages (pn_prof kinds >= 3000; the library reports their algorithmic vector instructions per lane-element)
VALU_STAGE_NAMES = {
    3001: ("one-hidden-layer head forward (k_pairsum_rowdot)", "add + max + fma per pair and hidden column"),
    3002: ("one-hidden-layer head backward reductions (k_pair_mask_reduce_fused<rank-1>)", "8 vector instructions per pair and hidden column"),
}
# 78.6 T lane-operations/s: 256 CUs x 4 SIMDs x 16 lanes x 2 (packed f32: v_pk_add_f32 / v_pk_fma_f32 do two per lane and clock -
# the rate behind the chip's 157.3 TFLOP/s vector-f32 figure, which counts an FMA as 2) at 2.4 GHz.  (Round 5's first run priced the
# stages against the unpacked 39.3 T and read 1.07: hipcc packs the adds and FMAs of k_pairsum_rowdot.)
VALU_PEAK_TOPS = 256 * 4 * 16 * 2 * 2.4e9 / 1e12
# ... but fmaxf has no packed form on gfx9: the one-hidden-layer forward's add + max + fma mix issues 3 operations in 2 slots
# (0.5 + 1 + 0.5) -> 39.3 T slots/s x 3 / 2 = 59 T operations/s is the rate THAT mix can reach; kinds without an
# entry here are priced at the packed rate (stated in each block as `peak_convention`)
VALU_MIX_PEAK_TOPS = {3001: 256 * 4 * 16 * 2.4e9 * 1.5 / 1e12}
F32_MFMA_PEAK_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: Peak FP32 (matrix)
BF16_MFMA_PEAK_TFLOPS = 2500.0  # same table: Peak BF16 MFMA, dense
HBM_PEAK_TBPS = 8.0  # same guide: HBM3E spec (measured copy rate there: 6.29 TB/s)
BUCKETS = (128, 256, 512, 1024, 2048)


def build_model(device, seed=42, unit_scale_weights=False, output_mlp_num_layers=3):
    import torch

    from protnote_amd.models.ProtNote import ProtNote
    from protnote_amd.models.protein_encoders import ProteInfer

    torch.manual_seed(seed)
    # configs/base_config.yaml: embed_sequences_params + params (PROJECTION_HEAD_*, OUTPUT_MLP_*, FEATURE_FUSION)
    enc = ProteInfer(num_labels=32102, input_channels=20, output_channels=1100, kernel_size=9,
                     activation=torch.nn.ReLU, dilation_base=3, num_resnet_blocks=5, bottleneck_factor=0.5)
    model = ProtNote(protein_embedding_dim=1100, label_embedding_dim=1024, latent_dim=1024, sequence_encoder=enc,
                     output_mlp_hidden_dim_scale_factor=3, output_mlp_num_layers=output_mlp_num_layers,
                     outout_mlp_add_batchnorm=True, projection_head_num_layers=4, projection_head_hidden_dim_scale_factor=3,
                     label_embedding_noising_alpha=20.0, feature_fusion="concatenation", temperature=0.07)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():  # random BN statistics/affine so activations and logits are O(1)
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.1)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) * 1.5 + 0.5)
        if unit_scale_weights:  # N(0, (1.6/sqrt(fan_in))^2) weights: O(1) logits instead of the ~1e-2 of default init
            for m in model.modules():
                if isinstance(m, (torch.nn.Linear, torch.nn.Conv1d)):
                    m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (1.6 / m.weight[0].numel() ** 0.5))
    for n, p in model.named_parameters():
        if n.startswith("sequence_encoder"):
            p.requires_grad = False  # TRAIN_SEQUENCE_ENCODER: False
    return model.to(device)


def synthetic_batch(B, L, NL, device, seed, ragged=False):
    import torch

    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, 20, (B, L), generator=g)
    onehots = torch.nn.functional.one_hot(ids, 20).permute(0, 2, 1).float().contiguous()
    return {
        "sequence_onehots": onehots.to(device),
        # SURVEY 8d variant: lengths ~ U[64, L] padded to L (the pad residues are masked by the kernels)
        "sequence_lengths": (torch.randint(min(64, L), L + 1, (B,), generator=g) if ragged
                             else torch.full((B,), L, dtype=torch.int64)).to(device),
        "label_embeddings": torch.randn(NL, 1024, generator=g).to(device),
        "label_token_counts": torch.randint(3, 40, (NL,), generator=g).to(device),
        "label_multihots": (torch.rand(B, NL, generator=g) < 1.6e-3).to(torch.int64).to(device),
    }


def _cpu_sample(threads, B=None):
    """One oracle train step on the bounded sample; returns (pairs, seconds)."""
    import torch

    from oracle import protnote_oracle as O
    from tests.helpers import random_encoder_sd, random_head_sd

    torch.set_num_threads(threads)
    gen = torch.Generator().manual_seed(0)
    ecfg = dict(num_labels=8, input_channels=20, output_channels=1100, kernel_size=9, dilation_base=3,
                num_resnet_blocks=5, bottleneck_factor=0.5)
    sd = {"sequence_encoder." + k: v for k, v in random_encoder_sd(ecfg, gen).items()}
    sd.update(random_head_sd(gen, 1100, 1024, 1024, 3072, 4, 3072, 3))
    B0, L, NL = CPU_SAMPLE
    B = B or B0
    ids = torch.randint(0, 20, (B, L), generator=gen)
    x = torch.nn.functional.one_hot(ids, 20).permute(0, 2, 1).float().contiguous()
    lens = torch.full((B,), L, dtype=torch.int64)
    lab = torch.randn(NL, 1024, generator=gen)
    y = (torch.rand(B, NL, generator=gen) < 1.6e-3).to(torch.int64)
    u = torch.rand(NL, 1024, generator=gen)
    cnt = torch.full((NL,), 5)
    t0 = time.time()
    O.train_step(sd, x, lens, lab, y, loss="BCE", noise_alpha=20.0, noise_u=u, label_token_counts=cnt)
    return B * NL, time.time() - t0


CPU_SAMPLE = (4, 512, 32102)  # SURVEY 8d / BASELINE.md 3: the reference materialises [B*N_L, 2d], so B = 4 at the real N_L
CPU_BUDGET_S = 65.0


def effective_cpus():
    """CPUs this process can really use: the affinity mask AND the cgroup's CFS quota.  The GPU boxes of this pool show 256
    hardware threads with `cpu.max` = 1600000 100000 - sixteen CPUs' worth of time (gpurun_out/r06f/cpu_probe.txt): more threads
    than that are throttled, which is why the all-cores legs of rounds 3-5 never finished."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota:
        n = min(n, max(1, int(math.ceil(quota))))
    return n, quota


def cpu_leg_threads(eff):
    """Thread counts of the cpu_baseline legs: all and twice the CPUs the process can really use, then - budget permitting - four
    times (PN_CPU_THREADS: one explicit count)."""
    if os.environ.get("PN_CPU_THREADS"):
        return [max(1, int(os.environ["PN_CPU_THREADS"]))]
    return sorted({max(1, eff), max(1, 2 * eff), max(1, 4 * eff)})


def _cpu_legs_main(threads_list, budget):
    """Child process of cpu_baseline: the B = 2 half-sample at the first two thread counts (one after the other: the CPU quota
    is one pool), the B = 4 sample at the faster of them, then the remaining thread counts at B = 2 while the budget lasts;
    one JSON line per finished sample."""
    t_start = time.time()
    best, slowest = None, 0.0

    def leg(t):
        nonlocal best, slowest
        pairs, dt = _cpu_sample(t, 2)
        print(json.dumps({"threads": t, "B": 2, "pairs": pairs, "seconds": dt}), flush=True)
        slowest = max(slowest, dt)
        if best is None or pairs / dt > best[1]:
            best = (t, pairs / dt)

    for t in threads_list[:2]:
        leg(t)
    pairs, dt = _cpu_sample(best[0], CPU_SAMPLE[0])
    print(json.dumps({"threads": best[0], "B": CPU_SAMPLE[0], "pairs": pairs, "seconds": dt}), flush=True)
    for t in threads_list[2:]:
        if budget - (time.time() - t_start) < 1.3 * slowest:
            print(json.dumps({"threads": t, "skipped": "budget"}), flush=True)
            continue
        leg(t)


def cpu_baseline(budget=CPU_BUDGET_S):
    """Oracle train step (reference algorithm restated, f32, torch-CPU; pinned to reference golden vectors) on a bounded
    sample of the same workload at the QUOTED label set: L = 512, N_L = 32102, full-width model (the whole W_l recompute over
    the real label table is in it).  One child process, one wall-clock budget: legs at one and two times the CPUs the process
    can really use (affinity and cgroup quota, effective_cpus) run the B = 2 half-sample one after the other, the faster thread
    count then runs the B = 4 sample (128 k pairs), and a four-times leg follows if the budget still holds it.  `value` = the
    B = 4 figure (the best B = 2 leg if B = 4 did not finish: fewer pairs over the same W_l cost, i.e. lower, never
    flattering); `cores` = its threads."""
    total = os.cpu_count() or 1
    eff, quota = effective_cpus()
    B4, L, NL = CPU_SAMPLE
    threads = cpu_leg_threads(eff)
    env = {k: v for k, v in os.environ.items() if k not in ("OMP_NUM_THREADS", "MKL_NUM_THREADS")}
    code = "import sys; sys.path.insert(0, %r); import bench; bench._cpu_legs_main(%r, %r)" % (ROOT, threads, float(budget) - 6.0)
    t0 = time.time()
    out, note = "", None
    try:
        pr = subprocess.Popen([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, env=env)
        try:
            out, _ = pr.communicate(timeout=budget)
        except subprocess.TimeoutExpired:
            pr.kill()
            note = f"stopped at the {budget:.0f} s budget"
            try:
                out, _ = pr.communicate(timeout=5)
            except Exception:  # noqa: BLE001
                pass
    except Exception as e:  # noqa: BLE001 - the baseline must not take the bench line down
        note = f"failed: {str(e)[:100]}"
    done = []
    for ln in (out or "").splitlines():
        try:
            done.append(json.loads(ln))
        except ValueError:
            pass
    legs, skipped = {}, []
    for t in threads:
        r = [d for d in done if d["threads"] == t and d.get("B") == 2]
        if r:
            legs[str(t)] = {"threads": t, "B": 2, "value": r[0]["pairs"] / r[0]["seconds"], "seconds": r[0]["seconds"]}
        elif any(d["threads"] == t and d.get("skipped") for d in done) or (t in threads[2:] and note is None):
            skipped.append(t)  # the optional leg: not started because the budget would not hold it
        else:
            legs[str(t)] = {"threads": t, "B": 2, "value": None, "seconds": None, "note": note or "not reached"}
    full = [d for d in done if d.get("B") == B4]
    base = {"unit": "protein-label pairs/s", "kind": "port", "host_cores": total, "usable_cpus": eff,
            "cpu_quota": quota, "legs": legs, "legs_not_started": skipped, "wall_seconds": time.time() - t0}
    if full:
        f = full[-1]
        legs[f"{f['threads']} (B={B4})"] = {"threads": f["threads"], "B": B4, "value": f["pairs"] / f["seconds"], "seconds": f["seconds"]}
        best = legs[f"{f['threads']} (B={B4})"]
    else:
        ok = [v for v in legs.values() if v["value"]]
        if not ok:
            return {"value": None, "cores": None, **base, "sample": f"no leg finished ({note})"}
        best = max(ok, key=lambda v: v["value"])
    return {"value": best["value"], "cores": best["threads"], **base,
            "sample": f"1 oracle train step (fwd+bwd+clip+Adam), B={best['B']}, L={L}, N_L={NL} (the quoted label set), full-width "
                      f"model, {best['seconds']:.1f} s on {best['threads']} threads = the faster of the {'/'.join(map(str, threads[:2]))}-thread "
                      f"legs; the host shows {total} hardware threads, the cgroup grants {eff} CPUs"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(n):
    """`python bench.py --gpus N` without a torchrun environment: run N ranks of this script under
    torch.distributed.run on this node (one process per GPU, RCCL), and hand back its exit code."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC (RCCL across processes needs it on this driver)
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def gemm_kinds(prof):
    return {k: v for k, v in prof.items() if k < 2000}


def stages_block(prof, steps):
    """SURVEY 8d's HBM-bound stages, event-timed inside the timed region like the GEMM kinds: per stage the algorithmic
    bytes of a launch, its mean duration, TB/s and the fraction of the 8 TB/s HBM roofline."""
    out = {}
    for kind, (cnt, ms, nbytes) in sorted(prof.items()):
        if kind < 2000 or cnt == 0:
            continue
        if kind >= 3000:  # VALU-bound: lane-instructions against the vector unit's issue rate
            name, what = VALU_STAGE_NAMES.get(kind, (str(kind), ""))
            tops = nbytes / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            peak = VALU_MIX_PEAK_TOPS.get(kind, VALU_PEAK_TOPS)
            out[name] = {"bound": "valu", "launches_per_step": cnt / max(steps, 1), "lane_instructions_per_launch": nbytes / cnt,
                         "ms_per_launch": ms / cnt, "ms_per_step": ms / max(steps, 1), "achieved_Tops": round(tops, 2),
                         "peak_Tops": round(peak, 1), "frac": round(tops / peak, 4), "instructions": what,
                         "peak_convention": ("add + max + fma: fmaxf has no packed form, 3 operations per 2 issue slots"
                                             if kind in VALU_MIX_PEAK_TOPS else "packed f32 rate (2 operations per issue slot)")}
            continue
        name, what = STAGE_NAMES.get(kind, (str(kind), ""))
        tbps = nbytes / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        out[name] = {"bound": "hbm", "launches_per_step": cnt / max(steps, 1), "algorithmic_bytes_per_launch": nbytes / cnt,
                     "ms_per_launch": ms / cnt, "ms_per_step": ms / max(steps, 1), "achieved_TBps": round(tbps, 3),
                     "peak_TBps": HBM_PEAK_TBPS, "frac": round(tbps / HBM_PEAK_TBPS, 4), "bytes": what}
    return out


def family(prof):
    """Dominant family: launches that contract over the full pair grid with a 3072x3072 weight
    -> (TFLOP/s, launches, total ms, total flop)."""
    prof = gemm_kinds(prof)
    big = {k: v for k, v in prof.items() if v[0] > 0 and v[2] / v[0] > 1e12} or prof
    tot_ms = sum(v[1] for v in big.values())
    tot_fl = sum(v[2] for v in big.values())
    n_launch = sum(v[0] for v in big.values())
    return (tot_fl / (tot_ms * 1e-3) / 1e12 if tot_ms > 0 else 0.0), n_launch, tot_ms, tot_fl


def kernel_table(prof):
    out = {}
    for kind, (cnt, ms, fl) in sorted(gemm_kinds(prof).items()):
        out[KIND_NAMES.get(kind, str(kind))] = {
            "launches": cnt, "ms_total": round(ms, 3), "tflops": round(fl / (ms * 1e-3) / 1e12, 2) if ms > 0 else 0}
    return out


def roofline_block(prof, math_mode, kernel_note):
    ach, n_launch, tot_ms, tot_fl = family(prof)
    peak = F32_MFMA_PEAK_TFLOPS if math_mode == "f32" else BF16_MFMA_PEAK_TFLOPS
    blk = {"bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
           "kernel": kernel_note, "launches": n_launch, "avg_ms_per_launch": tot_ms / max(n_launch, 1),
           "flops_per_launch": tot_fl / max(n_launch, 1), "family_ms": tot_ms}
    if math_mode == "bf16":
        blk["note"] = "one bf16 MFMA product per flop over the dense bf16 peak (ceiling of frac: 1)"
    elif math_mode != "f32":
        blk["note"] = ("algorithmic (f32-equivalent) flops over the dense bf16 peak; each costs three bf16 MFMA "
                       "flops, so the ceiling of frac is 1/3")
    return blk


def similarity_bench(model, batch, dev, world, steps, sync, max_over_ranks):
    """FEATURE_FUSION: similarity (ProtNote.py:281-284) at the headline shape: train step (focal loss, the
    reference's default LOSS_FN) and eval forward of a model that shares the headline model's encoder.  The head itself is
    one [B x d] x [N_L x d]^T contraction: 2*d FLOP + 4 B written per pair - reported with its own roofline;
    the step around it is encoder- and W_l-bound."""
    import torch

    from protnote_amd import _lib
    from protnote_amd.models.ProtNote import ProtNote
    from protnote_amd.models.ProtNoteTrainer import train_step
    from protnote_amd.models.train_path import head_parameters
    from protnote_amd.utils.losses import get_loss
    from protnote_amd.utils.optim import FusedClipAdam

    torch.manual_seed(4242)
    sim = ProtNote(protein_embedding_dim=1100, label_embedding_dim=1024, latent_dim=1024,
                   sequence_encoder=model.sequence_encoder, projection_head_num_layers=4,
                   projection_head_hidden_dim_scale_factor=3, label_embedding_noising_alpha=20.0,
                   feature_fusion="similarity", temperature=0.07).to(dev).train()
    loss_fn = get_loss({"params": {"LOSS_FN": "FocalLoss", "FOCAL_LOSS_GAMMA": 2, "FOCAL_LOSS_ALPHA": -1,
                                   "LABEL_SMOOTHING": 0.0}}, bce_pos_weight=torch.tensor(1.0))
    opt = FusedClipAdam(head_parameters(sim), lr=3e-4, max_norm=1.0)
    B, NL = batch["label_multihots"].shape
    d = 1024
    for _ in range(2):
        train_step(sim, loss_fn, opt, batch)
    sync()
    _lib.prof_begin()
    t0 = time.time()
    for _ in range(steps):
        loss = train_step(sim, loss_fn, opt, batch)
    sync()
    t_train = max_over_ranks(time.time() - t0)
    tprof = _lib.prof_end()
    sim.eval()
    with torch.no_grad():
        for _ in range(2):
            sim(sequence_onehots=batch["sequence_onehots"], sequence_lengths=batch["sequence_lengths"],
                label_embeddings=batch["label_embeddings"])
        sync()
        _lib.prof_begin()
        t0 = time.time()
        for _ in range(steps):
            sim(sequence_onehots=batch["sequence_onehots"], sequence_lengths=batch["sequence_lengths"],
                label_embeddings=batch["label_embeddings"])
        sync()
        t_eval = max_over_ranks(time.time() - t0)
        eprof = _lib.prof_end()

    def head_roofline(prof, kinds, what):
        cnt = sum(prof[k][0] for k in kinds if k in prof)
        ms = sum(prof[k][1] for k in kinds if k in prof)
        fl = sum(prof[k][2] for k in kinds if k in prof)  # 2*d FLOP per pair and contraction
        ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        # each contraction also moves 4 B per pair (logits written / dlogits read): the HBM-side bound of the same launches
        return {"bound": "mfma", "kernel": what, "achieved": ach, "peak": F32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": ach / F32_MFMA_PEAK_TFLOPS, "launches_per_step": cnt / steps, "ms_per_step": ms / steps,
                "flop_per_pair": fl / steps / (B * NL), "bytes_per_pair": 4,
                "hbm_side": {"achieved_TBps": 4.0 * B * NL * cnt / max(ms * 1e-3, 1e-12) / 1e12, "peak_TBps": HBM_PEAK_TBPS}}

    out = {"workload": f"FEATURE_FUSION: similarity, per-GPU batch {B} x {NL} labels, d = {d}, focal loss; train step "
                       "fwd+bwd+clip+Adam and eval forward; shares the headline model's frozen encoder",
           "train": {"value": world * B * NL * steps / t_train, "unit": "pairs/s", "ms_per_step": t_train / steps * 1e3,
                     "final_loss": float(loss),
                     # forward cosine GEMM (nt:plain->scale) + the two backward contractions over the same grid
                     "roofline": head_roofline(tprof, [3, 900], "cosine GEMM fwd (nt:plain->scale) + the backward's dP^ / dL^ "
                                               "contractions (pn_similarity_bwd): 3 x 2*d FLOP per pair per step"),
                     "kernels": kernel_table(tprof), "stages": stages_block(tprof, steps)},
           "eval": {"value": world * B * NL * steps / t_eval, "unit": "pairs/s", "ms_per_forward": t_eval / steps * 1e3,
                    "roofline": head_roofline(eprof, [3], "cosine GEMM (gemm_nt E_SCALE_RC: row norm x col norm / T in the epilogue)"),
                    "kernels": kernel_table(eprof), "stages": stages_block(eprof, steps)}}
    del opt, sim
    return out


def one_hidden_layer_bench(model, batch, dev, world, steps, sync, max_over_ranks):
    """OUTPUT_MLP_NUM_LAYERS: 1 (configs/base_config.yaml:34; get_mlp ProtNote.py:337-378) at the headline shape: with the
    layer-1 factorisation this head has NO pair-grid GEMM - the forward is one fused pair-sum -> ReLU -> row-dot pass, the
    backward the rank-1 masked reductions (both VALU-bound, reported against the vector unit's issue rate); the step around
    them is the encoder and the projection MLPs.  Shares the headline model's frozen encoder."""
    import torch

    from protnote_amd import _lib
    from protnote_amd.models.ProtNote import ProtNote
    from protnote_amd.models.ProtNoteTrainer import train_step
    from protnote_amd.models.train_path import head_parameters
    from protnote_amd.utils.losses import get_loss
    from protnote_amd.utils.optim import FusedClipAdam

    torch.manual_seed(4343)
    m1 = ProtNote(protein_embedding_dim=1100, label_embedding_dim=1024, latent_dim=1024, sequence_encoder=model.sequence_encoder,
                  output_mlp_hidden_dim_scale_factor=3, output_mlp_num_layers=1, outout_mlp_add_batchnorm=True,
                  projection_head_num_layers=4, projection_head_hidden_dim_scale_factor=3, label_embedding_noising_alpha=20.0,
                  feature_fusion="concatenation").to(dev).train()
    loss_fn = get_loss({"params": {"LOSS_FN": "BCE"}}, bce_pos_weight=torch.tensor(1.0))
    opt = FusedClipAdam(head_parameters(m1), lr=3e-4, max_norm=1.0)
    B, NL = batch["label_multihots"].shape
    for _ in range(2):
        train_step(m1, loss_fn, opt, batch)
    sync()
    _lib.prof_begin()
    t0 = time.time()
    for _ in range(steps):
        loss = train_step(m1, loss_fn, opt, batch)
    sync()
    t_train = max_over_ranks(time.time() - t0)
    tprof = _lib.prof_end()
    m1.eval()
    with torch.no_grad():
        for _ in range(2):
            m1(sequence_onehots=batch["sequence_onehots"], sequence_lengths=batch["sequence_lengths"],
               label_embeddings=batch["label_embeddings"])
        sync()
        _lib.prof_begin()
        t0 = time.time()
        for _ in range(steps):
            m1(sequence_onehots=batch["sequence_onehots"], sequence_lengths=batch["sequence_lengths"],
               label_embeddings=batch["label_embeddings"])
        sync()
        t_eval = max_over_ranks(time.time() - t0)
        eprof = _lib.prof_end()

    def head_roof(prof):  # the dominant head kernel of this configuration: the VALU-bound pair passes
        st = {k: v for k, v in stages_block(prof, steps).items() if v.get("bound") == "valu"}
        ops = sum(v["lane_instructions_per_launch"] * v["launches_per_step"] for v in st.values())
        ms = sum(v["ms_per_step"] for v in st.values())
        ach = ops / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        # time-weighted peak of the stages in the block (each priced at the rate its instruction mix can reach)
        peak = ops / max(sum(v["lane_instructions_per_launch"] * v["launches_per_step"] / v["peak_Tops"] for v in st.values()), 1e-30)
        return {"bound": "valu", "achieved": ach, "peak": peak, "unit": "T lane-operations/s",
                "frac": ach / peak, "ms_per_step": ms, "kernel": "k_pairsum_rowdot (+ k_pair_mask_reduce_fused<rank-1> in training)"}

    out = {"workload": f"OUTPUT_MLP_NUM_LAYERS: 1, per-GPU batch {B} x {NL} labels, h = 3072, BCE; train step fwd+bwd+clip+Adam and "
                       "eval forward (label projection cached); no pair-grid GEMM exists in this configuration",
           "train": {"value": world * B * NL * steps / t_train, "unit": "pairs/s", "ms_per_step": t_train / steps * 1e3,
                     "final_loss": float(loss), "dtype": "f32", "roofline": head_roof(tprof), "kernels": kernel_table(tprof),
                     "stages": stages_block(tprof, steps)},
           "eval": {"value": world * B * NL * steps / t_eval, "unit": "pairs/s", "ms_per_forward": t_eval / steps * 1e3,
                    "dtype": "f32", "roofline": head_roof(eprof), "kernels": kernel_table(eprof), "stages": stages_block(eprof, steps)}}
    del opt, m1
    return out


def zero_shot_batches(seqs_per_rank, batch, rank, world, dev, seed=5):
    """configs[4] workload, weak scaling: `seqs_per_rank` x world sequences, lengths log-uniform in [32, 2048], padded
    to their bucket.  SEQUENCES are dealt to the ranks (not batches): within every length bucket rank r takes rows
    r, r + world, ... - the reference's rank-strided sampler (samplers.py:61,111) applied per bucket, so every rank
    holds the same mix of lengths (+-1 sequence per bucket) and no rank idles.  A rank then batches its share of a
    bucket in groups of `batch`.  Returns (batches, residues of the whole job, sequences of the whole job, this rank's
    sequences)."""
    import torch

    n_seq = seqs_per_rank * world
    g = torch.Generator().manual_seed(seed)
    lens = torch.exp(torch.rand(n_seq, generator=g) * (math.log(2048) - math.log(32)) + math.log(32)).long().clamp(32, 2048)
    ids = torch.randint(0, 20, (n_seq, 2048), generator=g)
    batches, mine_total = [], 0
    for bi, bmax in enumerate(BUCKETS):
        lo = BUCKETS[bi - 1] if bi else 0
        # (the bucket index rotates who takes row 0, so the remainders do not all land on rank 0)
        rows = torch.nonzero((lens > lo) & (lens <= bmax)).flatten()[(rank + bi) % world::world]
        mine_total += len(rows)
        for s in range(0, len(rows), batch):
            r = rows[s:s + batch]
            x = torch.nn.functional.one_hot(ids[r, :bmax], 20).permute(0, 2, 1).float().contiguous()
            for kk, i in enumerate(r):
                x[kk, :, lens[i]:] = 0
            batches.append((x.to(dev), lens[r].to(dev)))
    return batches, int(lens.sum()), n_seq, mine_total


HEADLINE_MAX_BYTES = 4096  # the driver parses bench.py's LAST stdout line; r04's 24 kB line was not parsed
DETAIL_PATH = os.path.join(ROOT, "bench_detail.json")


def _sig(x, n=6):
    """Floats to n significant digits (the compact line carries numbers, not noise)."""
    if isinstance(x, float):
        return float(f"{x:.{n}g}") if math.isfinite(x) else None
    return x


def _mode_line(blk, ms_key="ms_per_step"):
    """One-liner of a sub-benchmark block: value, ms_per_step, dtype, roofline.frac only."""
    if not blk:
        return None
    roof = blk.get("roofline") or {}
    out = {"value": _sig(blk.get("value")), "ms_per_step": _sig(blk.get(ms_key, blk.get("ms_per_step")))}
    if blk.get("dtype"):
        out["dtype"] = blk["dtype"]
    if roof.get("frac") is not None:
        out["roofline_frac"] = _sig(roof["frac"], 4)
    return out


def headline(full):
    """The compact (<= HEADLINE_MAX_BYTES) object printed as the LAST stdout line: the contract keys, `roofline`,
    `cpu_baseline` and a `modes` block of one-liners.  Everything else (`kernels`, `stages`, per-rank lists, notes) lives in
    bench_detail.json and on an earlier stdout line."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data")
    out = {k: _sig(full[k]) for k in keep if k in full}
    cfg = full.get("config", {})
    out["config"] = {"workload": "configs[2] train step fwd+bwd+clip+Adam, BCE, frozen ProteInfer encoder"
                     if "frozen encoder" in cfg.get("workload", "") else "configs[2] train step, trainable encoder",
                     **{k: cfg[k] for k in ("global_batch", "seq_len", "n_labels", "parallelism") if k in cfg}}
    r = full.get("roofline", {})
    out["roofline"] = {k: _sig(r.get(k)) for k in ("bound", "achieved", "peak", "unit", "frac", "launches",
                                                    "avg_ms_per_launch", "flops_per_launch", "traffic", "traffic_stale")}
    out["roofline"]["kernel"] = (r.get("kernel") or "")[:80]
    c = full.get("cpu_baseline")
    if c:
        out["cpu_baseline"] = {"value": _sig(c["value"]), "unit": c["unit"], "cores": c["cores"], "kind": c["kind"],
                               "host_cores": c.get("host_cores"), "sample": c["sample"][:160]}
    def opt(fn):
        """Optional blocks must never cost the contract keys (a KeyError / TypeError here once left the 24 kB detail
        line as the last stdout line): whatever a block lacks, it is skipped."""
        try:
            fn()
        except Exception:  # noqa: BLE001
            pass

    modes = {}

    def put(name, blk, ms_key="ms_per_step", **over):
        line = _mode_line(blk, ms_key)
        if line:
            modes[name] = {**line, **over}

    opt(lambda: put("fast_mode", full.get("fast_mode"), dtype="bf16x3"))
    for k, v in (full.get("amp_backward") or {}).items():
        opt(lambda k=k, v=v: put("amp_backward." + k, v))
    opt(lambda: put("amp_full", full.get("amp_full")))
    for k in ("frozen_output_layer", "ragged_lengths"):
        opt(lambda k=k: put(k, full.get(k), dtype=full.get("dtype")))
    for k, v in (full.get("forward_only") or {}).items():
        if isinstance(v, dict):
            opt(lambda k=k, v=v: put("forward_only." + k, v, "ms_per_forward", dtype=(v.get("dtype") or k)[:48]))
    for mode, tables in (full.get("zero_shot") or {}).items():
        if isinstance(tables, dict) and mode in ("f32", "bf16x3", "bf16", "fp16x2"):
            for name, v in tables.items():
                def zs(mode=mode, name=name, v=v):
                    modes[f"zero_shot.{mode}.{name.split(' ')[0]}"] = {
                        "value": _sig(v.get("value")), "ms_per_step": _sig((v.get("seconds") or 0.0) * 1e3), "dtype": mode,
                        "roofline_frac": _sig((v.get("roofline") or {}).get("frac"), 4)}
                opt(zs)
    sh = full.get("similarity_head") or {}
    opt(lambda: put("similarity_head.train", sh.get("train"), dtype="f32"))
    opt(lambda: put("similarity_head.eval", sh.get("eval"), "ms_per_forward", dtype="f32"))
    oh = full.get("one_hidden_layer") or {}
    opt(lambda: put("one_hidden_layer.train", oh.get("train")))
    opt(lambda: put("one_hidden_layer.eval", oh.get("eval"), "ms_per_forward"))
    if modes:
        out["modes"] = modes
    if full.get("comm"):
        opt(lambda: out.update(comm={k: _sig(full["comm"].get(k)) for k in ("backend", "rccl_ranks", "replicas_in_sync",
                                                                           "ms_per_step_total", "share_of_step")}))
    for k in ("build_hash", "detail"):
        if k in full:
            out[k] = full[k]
    line = json.dumps(out, separators=(",", ":"))
    # never let the headline go unparsed again, and never lose a finished measurement to an assertion: shed optional blocks,
    # then free-text fields, until the line fits
    for shed in (lambda: out.pop("modes", None), lambda: out.pop("comm", None),
                 lambda: out.get("cpu_baseline", {}).update(sample=out.get("cpu_baseline", {}).get("sample", "")[:60]),
                 lambda: out["roofline"].update(kernel=out["roofline"]["kernel"][:30]),
                 lambda: out["config"].update(workload=out["config"]["workload"][:40])):
        if len(line) <= HEADLINE_MAX_BYTES:
            break
        shed()
        line = json.dumps(out, separators=(",", ":"))
    return line


def emit(full):
    """Detail to bench_detail.json and an EARLIER stdout line; the compact headline is the LAST stdout line."""
    full = dict(full)
    full["detail"] = "bench_detail.json (also the previous stdout line)"
    try:
        with open(DETAIL_PATH, "w") as f:
            json.dump(full, f, indent=1)
    except OSError as e:  # a read-only checkout must not cost the headline
        full["detail"] = f"previous stdout line (bench_detail.json not written: {e})"
    print(json.dumps({"bench_detail": full}), flush=True)
    print(headline(full), flush=True)


DUMP_PARAM_SAMPLE = 1 << 16  # elements kept of a larger parameter (fixed, seeded sample); smaller ones are kept whole
DUMP_SEED = 0


def dump_outputs(out_dir, loss, model, opt, counts):
    """--dump-outputs DIR: what a caller of the timed train step holds after the LAST timed step, as float32 .npy files:
      loss.npy                 [1]       the loss train_step returned
      params.npy               [n]       the updated trainable parameters (optimiser order)
      adam_exp_avg.npy         [n]       Adam's first moments at the same elements
      adam_exp_avg_sq.npy      [n]       Adam's second moments at the same elements
      bn_running_stats.npy     [m]       running_mean then running_var of every BatchNorm layer (model.modules() order)
      label_counts.npy         [3, N_L]  per-label TP / FN / FP accumulated by the loss pass over warmup + timed steps
    A parameter of more than DUMP_PARAM_SAMPLE elements contributes a sorted sample of that many, drawn without replacement
    from a generator seeded with DUMP_SEED (the same elements on every run), so the files stay well under 64 MB."""
    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.default_rng(DUMP_SEED)
    base = opt.flat_w.data_ptr()
    idx = []
    for p in opt.params:  # each parameter is a view of opt.flat_w; its moments sit at the same offsets of flat_m / flat_v
        off, n = (p.data_ptr() - base) // opt.flat_w.element_size(), p.numel()
        pick = np.arange(n) if n <= DUMP_PARAM_SAMPLE else np.sort(rng.choice(n, DUMP_PARAM_SAMPLE, replace=False))
        idx.append(off + pick)
    idx = torch.from_numpy(np.concatenate(idx)).to(opt.flat_w.device)
    bn = [t for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d) for t in (m.running_mean, m.running_var)]
    out = {"loss": np.array([loss], dtype=np.float32),
           "params": opt.flat_w[idx],
           "adam_exp_avg": opt.flat_m[idx],
           "adam_exp_avg_sq": opt.flat_v[idx],
           "bn_running_stats": torch.cat([t.detach().float().reshape(-1) for t in bn]),
           "label_counts": counts}
    for name, a in out.items():
        a = a.detach().float().cpu().numpy() if isinstance(a, torch.Tensor) else a
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq-len", type=int, default=512)
    ap.add_argument("--labels", type=int, default=32102)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--math", choices=["f32", "bf16x3"], default=os.environ.get("PN_MATH_MODE", "f32"),
                    help="arithmetic of the pair-grid GEMMs: exact f32 MFMA (default) or split-bf16 products")
    ap.add_argument("--train-encoder", action="store_true",
                    help="TRAIN_SEQUENCE_ENCODER: True - the ProteInfer trunk is trained too (non-default workload)")
    ap.add_argument("--ragged-lengths", action="store_true", help="sequence lengths ~ U[64, L] padded to L")
    ap.add_argument("--no-fast-mode", action="store_true",
                    help="skip the extra bf16x3 measurement reported under 'fast_mode' when --math f32")
    ap.add_argument("--no-extra", action="store_true", help="skip the forward_only / zero_shot sub-benchmarks")
    ap.add_argument("--zero-shot-seqs", type=int, default=512,
                    help="sequences PER RANK in the zero_shot sub-benchmark (weak scaling, like the headline)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="after the timed steps, write what the last one left the caller (loss, updated parameters and "
                         "optimiser moments - a fixed sample of the large ones -, BatchNorm running statistics, label "
                         "counts) to DIR/<name>.npy in float32 (rank 0; see dump_outputs)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(self_launch(args.gpus))

    import torch
    import torch.distributed as dist

    from protnote_amd import _lib
    from protnote_amd.models.ProtNoteTrainer import train_step
    from protnote_amd.models.train_path import head_parameters
    from protnote_amd.utils import distributed as D
    from protnote_amd.utils.losses import get_loss
    from protnote_amd.utils.optim import FusedClipAdam

    rank, local, world = D.init_from_env()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU "
                         f"(python bench.py --gpus {args.gpus} does it itself when no torchrun env is set)")
    dry = os.environ.get("PN_SHARE_GPU") == "1"  # several ranks on one GPU over gloo: plumbing check only
    if world > 1:
        if dist.get_world_size() != args.gpus:
            raise SystemExit(f"process group has {dist.get_world_size()} ranks, --gpus {args.gpus}")
        if not dry and dist.get_backend() != "nccl":
            raise SystemExit(f"multi-GPU bench must run over RCCL (backend 'nccl'), got {dist.get_backend()!r}")
        if not dry and torch.cuda.device_count() < world:
            raise SystemExit(f"{world} ranks but {torch.cuda.device_count()} visible GPUs")
    dev = torch.device("cuda", torch.cuda.current_device())  # set by init_from_env (LOCAL_RANK)

    _lib.set_math_mode(args.math)
    model = build_model(dev, seed=42 + rank)  # deliberately different per rank: sync_initial_state must fix it
    model.train()
    loss_fn = get_loss({"params": {"LOSS_FN": "BCE"}}, bce_pos_weight=torch.tensor(1.0))
    params = list(head_parameters(model))
    if args.train_encoder:
        model.train_sequence_encoder = True
        for q in model.sequence_encoder.trunk_parameters():
            q.requires_grad = True
        params += list(model.sequence_encoder.trunk_parameters())
    opt = FusedClipAdam(params, lr=3e-4, max_norm=1.0)
    if world > 1:
        D.sync_initial_state(model, opt)  # DDP-construction semantics: rank 0's weights / buffers everywhere
    B, L, NL = args.batch, args.seq_len, args.labels
    batch = synthetic_batch(B, L, NL, dev, seed=1000 + rank, ragged=args.ragged_lengths)
    counts = torch.zeros(3, NL, dtype=torch.float32, device=dev)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(x):
        if world > 1:
            t = torch.tensor([x], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())
        return x

    def per_rank(x):
        """[x of rank 0, x of rank 1, ...] on every rank."""
        if world > 1:
            t = torch.zeros(world, dtype=torch.float64, device=dev)
            t[rank] = float(x)
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            return [float(v) for v in t.tolist()]
        return [float(x)]

    def spread(xs):
        return {"min": min(xs), "max": max(xs), "per_rank": [round(v, 4) for v in xs]}

    def timed_train(steps, warmup, model=model, loss_fn=loss_fn, opt=opt, batch=batch):
        for _ in range(warmup):
            train_step(model, loss_fn, opt, batch, world_size=world, counts=counts)
        sync()
        D.comm_timing(world > 1)
        _lib.prof_begin()
        t0 = time.time()
        loss = None
        for _ in range(steps):
            loss = train_step(model, loss_fn, opt, batch, world_size=world, counts=counts)
        torch.cuda.synchronize()
        own = time.time() - t0  # this rank's own time to finish its K steps (before waiting for the others)
        sync()
        elapsed = time.time() - t0
        prof = _lib.prof_end()
        comm = D.comm_stats() if world > 1 else None
        D.comm_timing(False)
        if comm is not None:
            # replicas must hold the same weights after K all-reduced steps: compare a checksum of the flat weight block
            ck = per_rank(float(opt.flat_w.double().sum().item()))
            comm["_replicas"] = {"replicas_in_sync": all(v == ck[0] for v in ck), "flat_w_checksum_per_rank": ck,
                                 "own_seconds_before_barrier": spread(per_rank(own))}
        return max_over_ranks(elapsed), prof, float(loss.item()), comm

    def timed_eval(fn, steps, warmup):
        with torch.no_grad():
            for _ in range(warmup):
                fn()
            sync()
            _lib.prof_begin()
            t0 = time.time()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            own = time.time() - t0
            sync()
            elapsed = time.time() - t0
        return max_over_ranks(elapsed), _lib.prof_end(), spread(per_rank(own))

    # ------------------------------------------------------------------ headline: train step
    elapsed, prof, loss_val, comm = timed_train(args.steps, args.warmup)
    if args.dump_outputs and rank == 0:  # before the sub-benchmarks below train the same model further
        dump_outputs(args.dump_outputs, loss_val, model, opt, counts)
    fast = None
    if args.math == "f32" and not args.no_fast_mode:  # same workload once more on the opt-in bf16x3 arithmetic
        # (sub-benchmarks run a bounded number of steps: the default driver invocation is 20 + 5 of the 6.6 s headline step, and
        #  the whole run has to stay inside a few minutes)
        n_fast, w_fast = max(1, min(args.steps, 10)), max(1, min(args.warmup, 2))
        _lib.set_math_mode("bf16x3")
        f_elapsed, f_prof, f_loss, _ = timed_train(n_fast, w_fast)
        _lib.set_math_mode("f32")
        fast = {"math": "bf16x3 (f32 operands split into bf16 hi+lo, 3 bf16 MFMAs per product, f32 accumulate)",
                "value": world * B * NL * n_fast / f_elapsed, "unit": "pairs/s", "steps": n_fast,
                "ms_per_step": f_elapsed / n_fast * 1e3, "final_loss": f_loss,
                "roofline": roofline_block(f_prof, "bf16x3", "pair-grid 3072x3072 bf16x3 GEMM family"),
                "kernels": kernel_table(f_prof)}

    # the same step with the reference's AMP-class backward: forward as in `fast_mode` (bf16x3, logits bit-identical to
    # it), the four backward pair-grid GEMMs of the hidden layers on ONE bf16 product with f32 accumulation
    # (pn_set_backward_math(1); the reference trains under fp16 autocast, ProtNoteTrainer.py:728-738)
    amp = None
    if args.math == "f32" and not args.no_fast_mode:
        n_amp, w_amp = max(1, min(args.steps, 6)), 1
        amp = {}
        for fwd_mode in ("bf16x3", "f32"):
            _lib.set_math_mode(fwd_mode)
            _lib.set_backward_math("bf16")
            try:
                a_elapsed, a_prof, a_loss, _ = timed_train(n_amp if fwd_mode == "bf16x3" else max(1, min(n_amp, 3)), w_amp)
            finally:
                _lib.set_backward_math("same")
                _lib.set_math_mode("f32")
            n_run = n_amp if fwd_mode == "bf16x3" else max(1, min(n_amp, 3))
            one = {k: v for k, v in gemm_kinds(a_prof).items() if 1500 <= k < 2000 and v[0] > 0}
            one_ms, one_fl = sum(v[1] for v in one.values()), sum(v[2] for v in one.values())
            one_n = sum(v[0] for v in one.values())
            ach = one_fl / (one_ms * 1e-3) / 1e12 if one_ms > 0 else 0.0
            amp["forward_" + fwd_mode] = {
                "math": f"forward {fwd_mode} (logits bit-identical to that mode); backward dW_l / dh_l GEMMs of the hidden "
                        "layers: operands rounded to bf16, one MFMA product, f32 accumulation",
                "dtype": f"forward {fwd_mode}, backward GEMMs bf16 x bf16 -> f32",
                "value": world * B * NL * n_run / a_elapsed, "unit": "pairs/s", "ms_per_step": a_elapsed / n_run * 1e3,
                "steps": n_run, "final_loss": a_loss,
                "roofline": {"bound": "mfma", "achieved": ach, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                             "frac": ach / BF16_MFMA_PEAK_TFLOPS, "launches": one_n,
                             "avg_ms_per_launch": one_ms / max(one_n, 1), "flops_per_launch": one_fl / max(one_n, 1),
                             "kernel": "backward pair-grid GEMMs on one bf16 product (gemm_nt_bf16x3_kernel<.., NP = 1> / "
                                       "gemm_tn_bf16x3_kernel<.., NP = 1>): f32 operands converted while staging"},
                "kernels": kernel_table(a_prof)}

    # the reference's full mixed-precision class (ProtNoteTrainer.py:287,728-738: forward AND backward under autocast): as
    # `amp_backward.forward_bf16x3`, with the hidden layers' FORWARD pair-grid GEMMs on one bf16 product as well
    # (pn_set_forward_math(1)).  Opt-in, never the headline: its logits are held to torch's autocast(bfloat16) run of the
    # oracle, not to the 1e-3 bound (tests/test_hip_fwd_bf16.py)
    amp_full = None
    if args.math == "f32" and not args.no_fast_mode:
        n_run, w_amp = max(1, min(args.steps, 8)), 1
        _lib.set_math_mode("bf16x3")
        _lib.set_backward_math("bf16")
        _lib.set_forward_math("bf16")
        try:
            a_elapsed, a_prof, a_loss, _ = timed_train(n_run, w_amp)
        finally:
            _lib.set_forward_math("same")
            _lib.set_backward_math("same")
            _lib.set_math_mode("f32")

        def one_product(prof, pick):
            sel = {k: v for k, v in gemm_kinds(prof).items() if 1500 <= k < 2000 and v[0] > 0 and v[2] / v[0] > 5e11 and pick(k)}
            ms, fl, n = sum(v[1] for v in sel.values()), sum(v[2] for v in sel.values()), sum(v[0] for v in sel.values())
            ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
            return {"bound": "mfma", "achieved": ach, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": ach / BF16_MFMA_PEAK_TFLOPS, "launches": n, "avg_ms_per_launch": ms / max(n, 1),
                    "flops_per_launch": fl / max(n, 1), "family_ms": ms}

        # forward kinds: the generated-operand NT launches (1500 + 10 * {1: bn_relu, 2: pairsum}); backward: nt:plain (dh) + tn:*
        fwd_roof = one_product(a_prof, lambda k: (k - 1500) in (10, 20) or 1700 <= k < 1800)
        fwd_roof["kernel"] = "forward pair-grid GEMMs z_l = h_{l-1} W_l^T on one bf16 product (operands rounded while staging)"
        all_roof = one_product(a_prof, lambda k: True)
        all_roof["kernel"] = "all six full-grid 3072x3072 launches of the step (2 forward, 4 backward) on one bf16 product"
        amp_full = {"math": "encoder / W_p / W_l / layer-1 tables bf16x3; hidden pair-grid GEMMs forward AND backward: operands "
                            "rounded to bf16, one MFMA product, f32 accumulation; stored activations, BatchNorm, loss f32",
                    "dtype": "forward + backward pair-grid GEMMs bf16 x bf16 -> f32 (rest bf16x3 / f32)",
                    "value": world * B * NL * n_run / a_elapsed, "unit": "pairs/s", "ms_per_step": a_elapsed / n_run * 1e3,
                    "steps": n_run, "final_loss": a_loss, "roofline": all_roof, "forward_roofline": fwd_roof,
                    "kernels": kernel_table(a_prof), "stages": stages_block(a_prof, n_run)}

    # ------------------------------------------------------------------ sub-benchmarks (outside the headline region)
    extra = {}
    if not args.no_extra:
        n_var = max(1, min(args.steps, 2))
        # SURVEY 8d variant of the headline workload: sequence lengths ~ U[64, L] padded to L (the pads are masked inside
        # the conv kernels; the head's pair grid is unchanged)
        if not args.ragged_lengths:
            rb = synthetic_batch(B, L, NL, dev, seed=1000 + rank, ragged=True)
            r_el, r_prof, r_loss, _ = timed_train(n_var, 1, batch=rb)
            extra["ragged_lengths"] = {
                "workload": f"the headline train step with sequence lengths ~ U[64, {L}] padded to {L} (SURVEY 8d variant)",
                "value": world * B * NL * n_var / r_el, "unit": "pairs/s", "ms_per_step": r_el / n_var * 1e3,
                "steps": n_var, "valid_residue_fraction": float(rb["sequence_lengths"].float().mean().item()) / L,
                "final_loss": r_loss, "roofline": roofline_block(r_prof, args.math, "pair-grid 3072x3072 GEMM family"),
                "encoder_gemm_ms_per_step": sum(v[1] for k, v in gemm_kinds(r_prof).items() if k % 1000 == 31) / n_var}
            del rb
        # TRAIN_PROJECTION_HEAD: False (ProtNoteTrainer.py:216-222): output_layer.* frozen, W_p / W_l keep training.  The
        # frozen stack's two 155 TFLOP weight-gradient GEMMs (and its dgamma / dbeta / dw_out reductions) are not run.
        if not args.train_encoder:
            from protnote_amd.utils.configs import build_training

            cfg_f = {"params": {"LOSS_FN": "BCE", "BCE_POS_WEIGHT": 1, "OPTIMIZER": "Adam", "LEARNING_RATE": 3e-4,
                                "CLIP_VALUE": 1, "TRAIN_SEQUENCE_ENCODER": False, "TRAIN_PROJECTION_HEAD": False}}
            f_loss_fn, f_opt, _ = build_training(cfg_f, model)  # re-flattens the still-trainable parameters
            if world > 1:
                D.sync_initial_state(model, f_opt)
            fz_el, fz_prof, fz_loss, _ = timed_train(n_var, 1, loss_fn=f_loss_fn, opt=f_opt)
            fz_fam = family(fz_prof)
            extra["frozen_output_layer"] = {
                "workload": "the headline train step under TRAIN_PROJECTION_HEAD: False (output_layer.* frozen as the "
                            "reference freezes it; W_p / W_l trained)",
                "value": world * B * NL * n_var / fz_el, "unit": "pairs/s", "ms_per_step": fz_el / n_var * 1e3,
                "steps": n_var, "final_loss": fz_loss, "trainable_parameters": int(f_opt.flat_w.numel()),
                "family_tflop_per_step": fz_fam[3] / n_var / 1e12, "family_tflop_per_step_unfrozen": family(prof)[3] / args.steps / 1e12,
                "roofline": roofline_block(fz_prof, args.math, "pair-grid 3072x3072 GEMM family"),
                "kernels": kernel_table(fz_prof)}
            for q in model.parameters():  # back to the headline configuration for what follows
                if q.dtype.is_floating_point:
                    q.requires_grad = True
            for n_, q in model.named_parameters():
                if n_.startswith("sequence_encoder"):
                    q.requires_grad = False
            del f_opt
        # the train-step activation store (2 x 101 GB) is not needed any more
        import protnote_amd

        model.__dict__.pop("_pn_train_save", None)
        protnote_amd.free_workspaces()
        torch.cuda.empty_cache()
        model.eval()
        # "bf16" = bf16x3 base arithmetic + the hidden pair-grid GEMMs on ONE bf16 product (pn_set_forward_math(1), opt-in)
        modes = [args.math] + (["bf16x3", "bf16"] if args.math == "f32" and not args.no_fast_mode else [])

        def set_mode(mode):
            _lib.set_math_mode("bf16x3" if mode == "bf16" else mode)
            _lib.set_forward_math("bf16" if mode == "bf16" else "same")

        DTYPES = {"bf16": "bf16x3 + hidden pair-grid GEMMs bf16 x bf16 -> f32 (one product)"}

        def fwd_only():
            model(sequence_onehots=batch["sequence_onehots"], sequence_lengths=batch["sequence_lengths"],
                  label_embeddings=batch["label_embeddings"])

        fo = {}
        for mode in modes:
            set_mode(mode)
            e_el, e_prof, e_spread = timed_eval(fwd_only, max(1, min(args.steps, 3)), 1)
            n = max(1, min(args.steps, 3))
            e_prof = gemm_kinds(e_prof)
            enc_ms = sum(v[1] for k, v in e_prof.items() if k % 1000 == 31)
            fo[mode] = {"value": world * B * NL * n / e_el, "unit": "pairs/s", "ms_per_forward": e_el / n * 1e3,
                        "encoder_share_of_gemm_time": enc_ms / max(sum(v[1] for v in e_prof.values()), 1e-9),
                        "rank_seconds": e_spread, "dtype": DTYPES.get(mode, mode),
                        "roofline": roofline_block(e_prof, mode, "pair-grid 3072x3072 GEMM family (eval forward)"),
                        "kernels": kernel_table(e_prof)}
        extra["forward_only"] = {"workload": f"BASELINE configs[1]: eval forward, per-GPU batch {B} x L={L}, {NL} labels, "
                                             "1 description per label", **fo}

        model.inference_descriptions_per_label = 2
        zb, residues, n_seq, n_mine = zero_shot_batches(args.zero_shot_seqs, 128, rank, world, dev)
        seqs_per_rank, batches_per_rank = per_rank(n_mine), per_rank(len(zb))
        gz = torch.Generator().manual_seed(7)
        tables = [("GO-2019 (32102 labels x 2 descriptions)", torch.randn(32102 * 2, 1024, generator=gz).to(dev)),
                  ("EC (5134 labels x 2 descriptions)", torch.randn(5134 * 2, 1024, generator=gz).to(dev))]
        zs = {}
        for mode in modes:
            set_mode(mode)
            res = {}
            for name, table in tables:  # the label table is swapped between the two timed passes, same model object
                model.set_label_table(name, table)  # resident in HBM under a name: the swap is a lookup

                def run(name=name):
                    for x, l in zb:
                        model(sequence_onehots=x, sequence_lengths=l, label_embeddings=name)

                with torch.no_grad():
                    if zb:
                        model(sequence_onehots=zb[0][0], sequence_lengths=zb[0][1], label_embeddings=name)
                # the same pass with W_l(L_f) recomputed per batch, as the reference does (ProtNote.py:270-271) - the
                # figure comparable with the reference; the headline `value` of each table below runs with the label
                # projection cached (computed once, in the untimed call above)
                nocache = None
                if mode == modes[0] or name.startswith("EC"):
                    model.label_projection_cache_size = 0
                    nocache, _, _ = timed_eval(run, 1, 0)
                    model.label_projection_cache_size = 4
                    with torch.no_grad():
                        if zb:
                            model(sequence_onehots=zb[0][0], sequence_lengths=zb[0][1], label_embeddings=name)
                z_el, z_prof, z_spread = timed_eval(run, 1, 0)
                z_prof = gemm_kinds(z_prof)
                gemm_ms = max(sum(v[1] for v in z_prof.values()), 1e-9)
                enc_ms = sum(v[1] for k, v in z_prof.items() if k % 1000 == 31)
                res[name] = {"value": n_seq * table.shape[0] / z_el, "unit": "pairs/s (description rows scored)",
                             "sequences_per_s": n_seq / z_el, "seconds": z_el, "rank_seconds": z_spread,
                             "encoder_share_of_gemm_time": enc_ms / gemm_ms,
                             "roofline": roofline_block(z_prof, mode, "pair-grid 3072x3072 GEMM family (eval chunks)")}
                if nocache is not None:
                    res[name]["seconds_without_label_projection_cache"] = nocache
                    res[name]["value_without_label_projection_cache"] = n_seq * table.shape[0] / nocache
            zs[mode] = res
        extra["zero_shot"] = {"workload": f"BASELINE configs[4]: {n_seq} sequences ({args.zero_shot_seqs} per rank, "
                                          f"{residues} residues), lengths log-uniform 32..2048 padded to buckets "
                                          f"{list(BUCKETS)}, batch 128, two descriptions per label ensembled, GO table then "
                                          "EC table swapped at run time; sequences dealt rank-strided within each bucket; "
                                          "`value` runs with L_e = W_l(table) cached per table (projected once, outside the "
                                          "timed pass), `value_without_label_projection_cache` recomputes it per batch as "
                                          "the reference does",
                              "sequences_per_rank": seqs_per_rank, "batches_per_rank": batches_per_rank, **zs}
        set_mode(args.math)
        model.inference_descriptions_per_label = 1
        extra["similarity_head"] = similarity_bench(model, batch, dev, world, max(2, min(args.steps, 5)), sync, max_over_ranks)
        extra["one_hidden_layer"] = one_hidden_layer_bench(model, batch, dev, world, max(2, min(args.steps, 5)), sync, max_over_ranks)

    if rank == 0:
        pairs = world * B * NL * args.steps
        traffic, traffic_src, traffic_stale = None, None, None
        for cand in ("r06_hbm_traffic.json", "r05_hbm_traffic.json", "r04_hbm_traffic.json", "r03_hbm_traffic.json", "r02_hbm_traffic.json"):
            tpath = os.path.join(ROOT, "profiles", cand)
            if args.math == "f32" and os.path.exists(tpath):
                try:
                    from protnote_amd.build import csrc_hash

                    doc = json.load(open(tpath))
                    traffic = doc.get("bytes_per_launch")
                    # the counters come from separate rocprofv3 --pmc passes of this command, not from this run: the file
                    # carries the hash of the kernel sources it was taken on
                    traffic_stale = doc.get("csrc_hash") != csrc_hash()
                    traffic_src = (f"profiles/{cand} (separate rocprofv3 --pmc passes of this command; not measured in this "
                                   f"run; kernel sources then {doc.get('csrc_hash')}, now {csrc_hash()})")
                    break
                except Exception:
                    traffic = None
        # SURVEY 8d also defines the head's work densely (the reference's own computation, joint tensor included):
        # 151.0 MFLOP per pair fwd+bwd; the factorised implementation issues 3 x 37.75 = 113.3 MFLOP per pair
        roof = roofline_block(prof, args.math,
                              "pair-grid 3072x3072 f32-MFMA GEMM family (gemm_nt_kernel / gemm_tn_kernel)"
                              if args.math == "f32" else
                              "pair-grid 3072x3072 bf16x3 GEMM family (gemm_nt_bf16x3_kernel / gemm_tn_bf16x3_kernel); "
                              "achieved = algorithmic (f32-equivalent) flops")
        roof.update({"traffic": traffic, "traffic_source": traffic_src, "traffic_stale": traffic_stale,
                     "whole_step_tflops_dense_definition": pairs * 151.0e6 / elapsed / 1e12,
                     "whole_step_tflops_issued": pairs * 113.26e6 / elapsed / 1e12,
                     "family_share_of_step": roof["family_ms"] / (elapsed * 1e3)})
        out = {
            "metric": "protein-label pairs/sec (fwd+bwd)", "value": pairs / elapsed, "unit": "pairs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32" if args.math == "f32" else "bf16x3 (f32 split into bf16 hi+lo, 3 MFMAs, f32 accumulate)",
            "data": "synthetic", "build_hash": _lib.build_hash(),
            "config": {"workload": "BASELINE configs[2]/[3]: train step fwd+bwd+clip+Adam, BCE loss, per-GPU batch "
                                   f"{B} x L={L}, {NL} GO-sized label set, random-init ProteInfer(1100ch,5 blocks)+"
                                   "ProtNote(concatenation head 3x3072, 4-layer projections), "
                                   + ("trainable encoder" if args.train_encoder else "frozen encoder"),
                       "global_batch": world * B, "seq_len": L, "n_labels": NL,
                       "parallelism": f"dp{world}" if world > 1 else "single", "final_loss": loss_val},
            "roofline": roof,
            "kernels": kernel_table(prof),
            # SURVEY 8d's HBM-bound stages of the SAME timed steps (events inside the timed region)
            "stages": stages_block(prof, args.steps),
        }
        if world > 1:
            replicas = (comm or {}).pop("_replicas", {})
            per_step = {k: {"calls_per_step": v["calls"] / args.steps, "bytes_per_call": v["bytes"] / max(v["calls"], 1),
                            "ms_per_step": v["ms"] / args.steps} for k, v in (comm or {}).items()}
            out["comm"] = {"backend": dist.get_backend(), "rccl_ranks": dist.get_world_size(), **replicas,
                           "collectives_rank0": per_step,
                           "ms_per_step_total": sum(v["ms_per_step"] for v in per_step.values()),
                           "share_of_step": sum(v["ms_per_step"] for v in per_step.values()) / (elapsed / args.steps * 1e3)}
        if fast is not None:
            out["fast_mode"] = fast
        if amp is not None:
            out["amp_backward"] = amp
        if amp_full is not None:
            out["amp_full"] = amp_full
        out.update(extra)
        if world == 1 and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline()
        emit(out)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
