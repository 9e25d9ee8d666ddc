#!/usr/bin/env python3
"""bench.py - headline benchmark of the NSC/CMRL hot path on MI355X.

Metric (BASELINE.json): 512-sample frames/s of one full train step (forward + losses + backward + TF1 Adam
[+ gradient all-reduce]) of the 2-codec CMRL cascade.  Workload = BASELINE config 3 (the north-star step):
2 codecs, strides [2] each (256 codes/frame, 32 bins), LPC-residual input fed as a tensor, 16x256-bin LSF
quantizer, joint "finetune_lpc" step (all scopes trainable, cmrl.py:392-511), batch 128 frames per GPU,
synthetic 16 kHz frames.  A "step" = one optimizer step over one batch resident in HBM.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 ... bench.py --gpus N ...

`python bench.py --gpus N` with N > 1 and no launcher environment starts the N ranks ITSELF: the parent (which never touches
a GPU: the device count comes from sysfs) runs `python -m torch.distributed.run --standalone --nproc-per-node N bench.py ...` as a
child process, relays rank 0's JSON line and exits with the child's return code; if the first set of ranks dies before printing,
one more set of fresh ranks runs without HSA_ENABLE_IPC_MODE_LEGACY (spawn_ranks).

After the untimed set-up steps and W warm-up steps exactly K steps are timed (in up to --passes passes).  --dump-outputs DIR
then writes what the last of them computed as DIR/<name>.npy (dump_outputs); inputs and initial parameters are seeded, so two
builds run with the same arguments can be compared output for output.

Prints ONE JSON line on rank 0.  `roofline` is for the dominant kernel class of the step (the persistent gated-block
data-gradient kernel, gated_block_dgrad2_kernel, unless another class takes a larger share), timed live with HIP events on
the launch stream over extra instrumented steps of the same workload; `cpu_baseline` times the float32 PyTorch-CPU oracle
(a port of the reference TF graph - TF itself is not installable) on a bounded sample on rank 0 at N=1.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BKD = [9, 9, 100, 20, 1, 2]
COEFF = [60.0, 10.0, 10.0, 0.0]          # --coeff_term '60 10 10 0' (README of the reference)
LR = 2e-4
RES_SCALAR = 1.0
MFLOP_PER_FRAME_JOINT = 1428.2           # 2 codecs x 3 x 238.04 MFLOP
PEAK_F32_MFMA_TFLOPS = 157.3             # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 (exact fp32)
PEAK_BF16_MFMA_TFLOPS = 2500.0           # MI355X_MICROARCH.md: dense bf16 MFMA; the split-operand kernels spend SIX bf16 products
PEAK_SPLIT6_TFLOPS = PEAK_BF16_MFMA_TFLOPS / 6.0   # per fp32-class product: their algorithmic FLOPs are priced against 1/6 of it
MIN_PASS_STEPS = 10                      # a timed pass stays long against the idle GPU the synchronize at each of its ends costs


def synth_batch(B, rank, device):
    """frames 0.03*N(0,1) clipped to [-1,1] times the training window; LSF inputs sorted U(0.03,3.1)."""
    rng = np.random.default_rng(1234 + rank)
    o = 32
    win = np.concatenate([np.hanning(2 * o - 1)[:o], np.ones(512 - 2 * o), np.hanning(2 * o - 1)[o - 1:]])
    x = (np.clip(0.03 * rng.standard_normal((B, 1, 512)), -1, 1) * win[None, None, :]).astype(np.float32)
    lpc = np.sort(rng.uniform(0.03, 3.1, (B, 16, 1)), axis=1).astype(np.float32)
    return torch.from_numpy(x).to(device), torch.from_numpy(lpc).to(device), x, lpc


# ---- the other BASELINE.json train configurations (parity-test cases; `--config N` times them too, the default and the
# driver's run is config 3).  name, codecs, strides per codec, LPC path, default batch per GPU, MFLOP per frame
CONFIGS = {
    2: ("BASELINE config 2: 1 codec (strides [2], 32-bin quantizer, quan + entropy terms, tau 0.3), time-domain frames, "
        "fwd+loss+bwd+TF1-Adam - run in fp32 (the reference's precision), not the bf16 the config names", 1, [2], False, 128, 714.1),
    3: (None, 2, [2], True, 128, MFLOP_PER_FRAME_JOINT),
    4: ("BASELINE config 4: 4-codec CMRL, every codec with two down-/up-sampling stages ('2 2': 128 codes, blocks at C = 100, 50, "
        "25), joint finetune step (cmrl.py:295-390 generalised to 4 codecs: quan weight coeff[2] x global batch, tau_i ent_i), "
        "fwd+loss+bwd+TF1-Adam", 4, [2, 2], False, 256, 3237.3),
}


def step_cfg_for(config, B, world):
    if config == 3:
        return step_cfg()
    n = CONFIGS[config][1]
    if config == 2:      # one_ae quan op (nsc_module:914-926): coeff[2] quan + tau ent, entropy of the global batch
        return dict(is_quan_on=1.0, c_time=COEFF[0], c_freq=COEFF[1], c_quan=[COEFF[2]], c_ent=[0.3], trainable=[True], lr=LR, slot=1,
                    quan_op=True)
    return dict(is_quan_on=1.0, c_time=COEFF[0], c_freq=COEFF[1], c_quan=[COEFF[2] * B * world] * n, c_ent=[0.3] * n,
                trainable=[True] * n, lr=LR, slot=1, quan_op=True)


def step_cfg():
    return dict(is_quan_on=1.0, c_time=COEFF[0], c_freq=COEFF[1], c_quan=[COEFF[2], COEFF[2]], c_ent=[0.0, 0.0],
                trainable=[True, True], lr=LR, slot=1, c_quan_lpc=COEFF[2], c_ent_lpc=0.0, train_lpc=True, quan_op=True, global_entropy=False)


def op_surface_leg(B, x_np, dev, steps=20, warmup=3):
    """The SAME codec step built from the drop-in op surface (nsc_amd.nn_core_operator / loss_terms_and_measures under torch autograd:
    what a user of the reference's nn_core_operator.py gets) beside the engine's figure for BASELINE config 2 (1 codec, strides [2],
    32 bins, quan + entropy terms), both timed here at the same batch.  The surface leg is forward + loss + backward (gradients of
    every variable); the engine's step also applies TF1-Adam."""
    from nsc_amd import loss_terms_and_measures as L
    from nsc_amd.engine import CascadeEngine
    from nsc_amd.neural_speech_coding_module import neuralSpeechCodingModule
    from nsc_amd.scope import VariableStore, set_store
    xe = torch.from_numpy(x_np[:B].copy()).to(dev)          # [B,1,512] (the engine's layout)
    xd = xe.reshape(B, 512, 1)                              # channels_last, like the reference's placeholder
    tgt = xd[:, :, 0].contiguous()
    st = VariableStore(device=str(dev))
    set_store(st)
    try:
        m = neuralSpeechCodingModule.__new__(neuralSpeechCodingModule)
        m._bottleneck_kernel_and_dilation = list(BKD)

        def surface_step():
            st.begin_pass()
            for v in st.vars.values():
                v.grad = None
            p, _, _, _, decoded, _, _, _ = m.computational_graph_end2end_quan_on(xd, True, 1.0, 32, "scope_1", [2])
            loss = (COEFF[0] * L.mse_loss(decoded, tgt) + COEFF[1] * L.mfcc_loss(decoded, tgt) + COEFF[2] * L.quan_loss(p)).sum() + \
                B * 0.3 * L.entropy_coding_loss(p)
            loss.backward()

        def timed(fn, n):
            fn(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n

        for _ in range(warmup):
            surface_step()
        torch.cuda.synchronize()
        t_surface_eager = timed(surface_step, steps)
        # ... and the same step captured once and replayed (torch's whole-network hipGraph recipe: static shapes, gradients written in
        # place by the replay) - what a user of the op surface does when the host is the bottleneck, and what the engine's figure uses
        t_surface_graph = None
        try:
            from nsc_amd.graph import capture_step
            gs = capture_step(surface_step, warmup=1)
            t_surface_graph = timed(gs, steps)
        except Exception as e:
            print(f"[bench] op_surface: graph capture of the surface step failed ({type(e).__name__}: {e}); eager figure stands", file=sys.stderr)
            torch.cuda.synchronize()
        t_surface = min(t_surface_eager, t_surface_graph) if t_surface_graph is not None else t_surface_eager
    finally:
        set_store(None)
    eng = CascadeEngine(B, 1, BKD, [[2]], [32], res_scalar=RES_SCALAR, scale_first=False, lpc=False, device=dev)
    cfg = step_cfg_for(2, B, 1)
    for _ in range(warmup):
        eng.train_step(xe, xe, cfg)
    torch.cuda.synchronize()
    t_eager = timed(lambda: eng.train_step(xe, xe, cfg), steps)
    t_graph = None
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            eng.train_step(xe, xe, cfg)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            eng.train_step(xe, xe, cfg)
        t_graph = timed(g.replay, steps)
    except Exception as e:                                  # the eager figure stands
        print(f"[bench] op_surface: engine graph capture failed ({e})", file=sys.stderr)
    t_eng = t_graph if t_graph is not None else t_eager
    return dict(frames_per_s=round(B / t_surface, 1), ms_per_step=round(1e3 * t_surface, 3),
                launch=("hipGraph replay of the captured autograd step" if t_surface_graph is not None and t_surface_graph <= t_surface_eager
                        else "eager (torch autograd tape)"),
                ms_per_step_eager=round(1e3 * t_surface_eager, 3),
                ms_per_step_graph=(round(1e3 * t_surface_graph, 3) if t_surface_graph is not None else None),
                work="forward + loss + backward of one codec through nn_core_operator / loss_terms_and_measures (no optimizer); round 6: the "
                     "blocks' forward on split operands, one image gather per pass, batched weight gradients at the end of the autograd pass (nsc_amd/ops.py)",
                engine_config2_frames_per_s=round(B / t_eng, 1), engine_config2_ms_per_step=round(1e3 * t_eng, 3),
                engine_config2_launch="hipGraph" if t_graph is not None else "eager",
                engine_config2_eager_ms_per_step=round(1e3 * t_eager, 3),
                engine_work="the same codec step + TF1-Adam", batch=B, steps=steps, frac_of_engine=round(t_eng / t_surface, 3))


def cpu_baseline(B, x_np, lpc_np, budget_s=24.0):
    """float32 PyTorch-CPU port of the same joint step (oracle/nsc_oracle_torch.py).  BASELINE.md section 3 protocol inside
    a bounded budget: warm-up steps, then up to 10 timed steps on all host cores (median step time), plus a 1-thread
    figure on a smaller batch.  Reported as a baseline only."""
    from oracle import nsc_oracle_torch as OT
    from tests._util import make_store
    ps = make_store(2, [[2], [2]], [32, 32], rand_bias=False, alpha=None, lpc=True)

    def runner(b):
        tp = OT.TorchParams(ps, dtype=torch.float32)
        plist = [tp.t[k] for k in tp.names]
        ms = [torch.zeros_like(p) for p in plist]
        vs = [torch.zeros_like(p) for p in plist]
        x = torch.tensor(np.ascontiguousarray(x_np[:b].transpose(0, 2, 1)))
        lpc = torch.tensor(lpc_np[:b])

        def one(t):
            t0 = time.perf_counter()
            for p in plist:
                p.grad = None
            outs, dec = OT.cascade_forward(x, tp, BKD, [[2], [2]], 1.0, True, RES_SCALAR, True)
            pl, _ = OT.scalar_softmax_quantization(lpc, tp.t["lpc_quan/alpha"], tp.t["lpc_quan/bins"], 1.0, True)
            OT.total_loss_sum(dec, x[:, :, 0], [o["p"] for o in outs], COEFF, 0.0, "finetune_lpc", (pl,)).backward()
            grads = [p.grad if p.grad is not None else torch.zeros_like(p) for p in plist]
            OT.adam_tf1_step_(plist, grads, ms, vs, t, LR)
            return time.perf_counter() - t0
        return one

    cores = torch.get_num_threads()
    t_start = time.perf_counter()
    # thread count: the graph is ~150 small convolutions, and oversubscribed intra-op pools lose to a few threads on this
    # host class - probe a short batch at several pool sizes and keep the fastest (that count is the `cores` reported)
    probe = {}
    for n in sorted({1, 8, 32, cores}):
        if n > cores:
            continue
        torch.set_num_threads(n)
        one16 = runner(16)
        one16(1)
        probe[n] = one16(2)
    best = min(probe, key=probe.get)
    torch.set_num_threads(best)
    one = runner(B)
    warm = one(1)
    times = []
    t_main = time.perf_counter()
    while len(times) < 10 and (len(times) < 3 or (time.perf_counter() - t_main) + warm < budget_s):
        times.append(one(len(times) + 2))
    med = float(np.median(times))
    torch.set_num_threads(1)
    one1 = runner(8)
    one1(1)
    t1 = one1(2)
    torch.set_num_threads(cores)
    return dict(value=B / med, unit="frames/s", cores=best, kind="port", timed_steps=len(times), host_threads_available=cores,
                thread_probe_s_per_16_frames={str(k): round(v, 3) for k, v in probe.items()},
                one_thread_frames_per_s=round(8 / t1, 3),
                sample=f"1 warm-up + {len(times)} timed joint train steps (median) of the same 2-codec CMRL config, batch {B}, "
                       f"float32 PyTorch-CPU restatement of the reference TF graph on {best} of {cores} host threads (fastest "
                       f"of a 1/8/32/{cores}-thread probe); {time.perf_counter() - t_start:.1f} s in all; 1-thread figure: batch 8")


def pass_sizes(steps, passes):
    """--steps K: K timed steps in all, in at most `passes` passes of near-equal length, each of at least MIN_PASS_STEPS steps
    unless K itself is smaller."""
    n = max(1, min(passes, steps // MIN_PASS_STEPS))
    return [steps // n + (i < steps % n) for i in range(n)]


DUMP_BYTES = 64 * 10 ** 6           # --dump-outputs: every file together, .npy headers included
DUMP_HEADER_BYTES = 4096            # reserved per file for its .npy header
DUMP_SEED = 20200504                # indices of the sample of an array too large for its share


def dump_outputs(d, arrays):
    """--dump-outputs: write every array (float32, as the step computed it) as d/<name>.npy.  The files stay within DUMP_BYTES in
    all: an array larger than its share of what is left is replaced by a fixed, seeded sample of its flat elements (sorted indices,
    the same for the same arguments on every run).  Returns {name: (shape written, whole)}."""
    os.makedirs(d, exist_ok=True)
    items = sorted(arrays.items(), key=lambda kv: kv[1].size)
    left = DUMP_BYTES - DUMP_HEADER_BYTES * len(items)
    out = {}
    for i, (name, a) in enumerate(items):
        a = np.ascontiguousarray(a, dtype=np.float32)
        share = left // (len(items) - i)
        whole = a.nbytes <= share
        if not whole:
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(a.size, share // a.itemsize, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(d, name + ".npy"), a)
        left -= a.nbytes
        out[name] = (a.shape, whole)
    return out


def step_outputs(eng, terms):
    """What a caller of the timed step receives after it: the loss terms train_step returns, the decoded frames of its forward pass,
    the gradients it computed and the parameters its Adam update left (flat buffers, the engine's layout).  A replayed hipGraph
    writes the same buffers the captured call returned."""
    t = {"decoded": eng.decoded, "loss_time": terms["time"], "loss_freq": terms["freq"], "params": eng.params, "grads": eng.grads}
    for c, q, e in zip(eng.codecs, terms["quan"], terms["ent"]):
        t[f"loss_quan_{c.scope}"] = q
        t[f"entropy_{c.scope}"] = e
    if terms.get("quan_lpc") is not None:
        t["loss_quan_lpc"] = terms["quan_lpc"]
    if terms.get("ent_lpc") is not None:
        t["entropy_lpc"] = terms["ent_lpc"]
    return {k: v.detach().cpu().numpy() for k, v in t.items()}


class _NullComm:
    """--dp-selftest: the data-parallel control flow of one rank with every collective a no-op (prices the segmentation)."""
    world, rank = 1, 0

    def allreduce_async(self, t, op=None):
        return None

    def allreduce_list(self, tensors):
        pass


def _count_gpus_sysfs():
    """GPUs of this node WITHOUT touching HIP / HSA (torch.cuda.device_count() initialises the runtime on ROCm builds without amdsmi):
    KFD topology nodes with a non-zero simd_count.  None when the topology is not readable (the children then report what they see)."""
    root = "/sys/class/kfd/kfd/topology/nodes"
    if not os.path.isdir("/sys/class/kfd"):
        return 0                               # no amdgpu compute driver on this machine
    try:
        n = 0
        for d in os.listdir(root):
            with open(os.path.join(root, d, "properties")) as f:
                for line in f:
                    if line.startswith("simd_count"):
                        n += int(line.split()[1]) > 0
                        break
        return n
    except OSError:
        return None


def _count_gpus_visible():
    """GPUs a child process of this one would SEE: the sysfs count ignores HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES and cgroup
    device limits, so ask a throw-away child (device_count() only - this parent still never touches a GPU).  None when the
    probe itself fails."""
    try:
        out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True,
                             timeout=300)
        return int(out.stdout.strip().splitlines()[-1]) if out.returncode == 0 else None
    except (OSError, ValueError, IndexError, subprocess.TimeoutExpired):
        return None


def spawn_ranks(n, argv):
    """--gpus N > 1 without a launcher: start N fresh ranks under torch.distributed.run as a CHILD process and relay rank 0's JSON
    line.  This parent never initialises a GPU (the device count comes from sysfs), nothing is exec'ed, and the rendezvous port is
    picked by the launcher itself (--standalone: a c10d store on a free loopback port - no bind / close / reuse race).
    First contact with RCCL: the children run with HSA_ENABLE_IPC_MODE_LEGACY=0 (dmabuf IPC, what this driver supports; already
    exported on the pool's boxes).  If they exit non-zero BEFORE rank 0 printed its line, ONE more set of fresh children is started
    with the variable unset - a new child process, not a restart of a process that touched a GPU - and the line says so."""
    backend = os.environ.get("NSC_DIST_BACKEND") or "nccl"
    ndev = _count_gpus_sysfs()
    if backend == "nccl" and (ndev is None or ndev >= n):
        nvis = _count_gpus_visible()           # (only when sysfs says there could be enough)
        if nvis is not None:
            ndev = nvis if ndev is None else min(ndev, nvis)
    if backend == "nccl" and ndev is not None and ndev < n:
        print(f"[bench] --gpus {n} needs {n} GPUs for RCCL (one rank per GPU) but this process can see {ndev}; nothing was launched.  "
              f"(NSC_DIST_BACKEND=gloo shares the visible GPU(s) between ranks: control-flow test only.)", file=sys.stderr)
        return 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           f"--nproc-per-node={n}", os.path.abspath(__file__)] + list(argv)

    def attempt(env, note):
        print(f"[bench] launching {n} ranks{note}: {' '.join(cmd)}", file=sys.stderr, flush=True)
        proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=None, text=True)
        line_json = None
        for line in proc.stdout:              # rank 0 prints the ONE JSON line; anything else goes to stderr untouched
            if line.lstrip().startswith("{") and '"metric"' in line:
                line_json = line.strip()
            else:
                sys.stderr.write(line)
        return proc.wait(), line_json

    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: RCCL's intra-node transport on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    rc, line_json = attempt(env, "")
    if rc != 0 and line_json is None and backend == "nccl" and os.environ.get("NSC_BENCH_NO_IPC_RETRY") is None:
        env2 = dict(env)
        env2.pop("HSA_ENABLE_IPC_MODE_LEGACY", None)
        env2["NSC_BENCH_LAUNCH_NOTE"] = "second set of ranks, HSA_ENABLE_IPC_MODE_LEGACY unset (the first set exited with %d before printing)" % rc
        print(f"[bench] the ranks exited with {rc} before printing a line; ONE more set of fresh ranks without HSA_ENABLE_IPC_MODE_LEGACY",
              file=sys.stderr, flush=True)
        rc, line_json = attempt(env2, " (retry)")
    if line_json is not None:
        print(line_json, flush=True)
    elif rc == 0:
        print("[bench] the ranks exited with 0 but printed no JSON line", file=sys.stderr)
        rc = 1
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="frames per GPU (BASELINE: 128; config 4: 256)")
    ap.add_argument("--config", type=int, default=3, choices=(2, 3, 4),
                    help="BASELINE.json configuration to time (3 = the headline 2-codec joint step; 2 and 4: the other train configs)")
    ap.add_argument("--follower", action="store_true",
                    help="config 3 only: time the FOLLOWER step instead of the joint one (SURVEY 8d: codec 1 frozen and forward-only, "
                         "codec 2 trains on its residual: cmrl.py:137-293; 952.2 MFLOP per frame)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--arith", choices=["split", "exact"], default=None,
                    help="arithmetic of the gated blocks' forward and weight gradients: split = bf16 matrix cores on fp32 operands split "
                         "into 3 bf16 pieces, 6 products, fp32 accumulate (the engine's default); exact = the fp32 matrix instruction")
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--passes", type=int, default=3,
                    help="at most this many timed passes the --steps steps are divided into, each of at least %d steps unless --steps is "
                         "smaller (value = the median pass)" % MIN_PASS_STEPS)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last of them computed (loss terms, decoded frames, gradients, updated "
                         "parameters) as DIR/<name>.npy in float32, %d MB at most in all (a fixed, seeded sample of a larger array); "
                         "rank 0 only" % (DUMP_BYTES // 10 ** 6))
    ap.add_argument("--dp-selftest", action="store_true",
                    help="N=1 only: run the data-parallel control flow (segmented hipGraph, collectives as no-ops) to price it")
    ap.add_argument("--dp-overlap", action="store_true",
                    help="data parallel: one gradient message per scope under the backward pass (splits the batched weight-gradient "
                         "launches: measured slower) instead of one message at the tail of the step")
    ap.add_argument("--prof-steps", type=int, default=3)
    ap.add_argument("--no-infer", action="store_true", help="skip the codec-forward us/frame measurement")
    ap.add_argument("--no-op-surface", action="store_true", help="skip the op-surface leg (a codec step built from nn_core_operator ops)")
    ap.add_argument("--no-overlap", action="store_true", help="weight-gradient kernels on the main stream (profiling)")
    ap.add_argument("--wgrad-waves", type=int, default=8)
    ap.add_argument("--no-split-wgrad", action="store_true")
    ap.add_argument("--no-batch-wgrad", action="store_true", help="debug: per-block weight-gradient launches instead of one deferred batch")
    ap.add_argument("--no-batch-conv-wgrad", action="store_true", help="debug: one weight-gradient launch per conv on the side stream instead of one deferred batched launch per kernel class")
    ap.add_argument("--unfused-wgrad", action="store_true", help="debug: per-conv weight gradients")
    ap.add_argument("--unfused-dgrad", action="store_true", help="debug: per-conv data-gradient launches instead of one fused kernel per gated block")
    ap.add_argument("--unfused-fwd", action="store_true", help="debug: per-conv forward/backward (no block fusion)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    from nsc_amd.dist import Comm
    from nsc_amd.engine import CascadeEngine
    comm = Comm()
    if comm.world != args.gpus:
        raise SystemExit(f"[bench] WORLD_SIZE {comm.world} != --gpus {args.gpus}: launch `python bench.py --gpus N` (it starts the "
                         f"ranks itself) or torch.distributed.run with --nproc-per-node equal to --gpus")
    ldev = comm.local_rank % torch.cuda.device_count()   # one GPU per rank on a real node; wraps only in single-GPU smoke tests
    torch.cuda.set_device(ldev)
    dev = torch.device("cuda", ldev)
    comm.preflight(dev)                                  # first contact with RCCL: a checked 4-float all-reduce, clear error
    wl_name, ncodec, strides_c, use_lpc, B_default, mflop_frame = CONFIGS[args.config]
    B = args.batch or B_default
    if args.config != 3:
        args.no_infer = args.no_cpu_baseline = True       # those legs belong to the headline configuration
    eng = CascadeEngine(B, ncodec, BKD, [list(strides_c)] * ncodec, [32] * ncodec, res_scalar=RES_SCALAR, scale_first=use_lpc,
                        lpc=use_lpc, device=dev)
    eng.overlap_wgrad = not args.no_overlap
    eng.wgrad_waves = args.wgrad_waves
    eng.split_wgrad = not args.no_split_wgrad
    eng.fused_wgrad = not args.unfused_wgrad
    eng.fused_dgrad = not args.unfused_dgrad
    eng.batch_wgrad = not args.no_batch_wgrad
    eng.batch_conv_wgrad = not args.no_batch_conv_wgrad
    eng.fused_fwd = not args.unfused_fwd
    if args.arith is not None:
        eng.split_fwd = eng.split_wgrad_arith = args.arith == "split"
        eng.split_conv = eng.split_conv and args.arith == "split"      # (laid out at construction: can only be switched off)
    split_on = bool(eng.split_fwd or eng.split_wgrad_arith or eng.split_dgrad or eng.split_conv)
    xd, lpcd, x_np, lpc_np = synth_batch(B, comm.rank, dev)
    cfg = step_cfg_for(args.config, B, comm.world)
    if args.follower:
        assert args.config == 3, "--follower is the second step of config 3"
        # neural_speech_coding_module._loss_cfgs(2, "follower"): only the newest scope trains, quan / entropy terms of the newest
        # codec only (cmrl.py:97-98, 106-113); tau 0.3 as in config 2 so that the entropy term (and, data-parallel, its histogram
        # all-reduce) is part of the step
        cfg = dict(is_quan_on=1.0, c_time=COEFF[0], c_freq=COEFF[1], c_quan=[0.0, COEFF[2]], c_ent=[0.0, 0.3], trainable=[False, True],
                   lr=LR, slot=1, quan_op=True)
        mflop_frame = 952.2                   # forward of both codecs + backward of the second (4 x 238.04)
        wl_name = ("BASELINE config 3, FOLLOWER step: 2-codec CMRL (strides [2], 32 bins) on fed LPC residual, codec 1 frozen "
                   "(forward only), codec 2 trains on its residual (quan + entropy terms of codec 2, tau 0.3), fwd+loss+bwd+TF1-Adam")
        args.no_infer = args.no_cpu_baseline = True
    if not use_lpc:
        lpcd = None
    dcomm = comm if comm.world > 1 else (_NullComm() if args.dp_selftest else None)
    eng.dp_overlap = bool(args.dp_overlap)

    last_terms = {}

    def step():
        last_terms.update(eng.train_step(xd, xd, cfg, lpc_x=lpcd, comm=dcomm))

    # C-ABI calls of one eager step (kernel dispatches per step come from the rocprof trace: profiles/*_step_timeline.txt)
    from nsc_amd import _lib as _nl, engine as _ne
    ncalls = [0]
    _chk = _nl.check
    def _counting(rc, what=""):
        ncalls[0] += 1
        return _chk(rc, what)
    step()                                   # allocates every buffer
    _ne.check = _counting
    step()
    _ne.check = _chk
    calls_per_step = ncalls[0]
    # The pair launches (two gated blocks per launch, neighbour flags between workgroups) need all their workgroups resident at
    # once.  If a neighbour wait timed out in these first steps on ANY rank (another process or a collective's kernel holding
    # compute units), all ranks switch to one launch per block BEFORE anything is captured or timed, and the line says so.
    torch.cuda.synchronize()
    pairs_note = None
    fake_to = os.environ.get("NSC_BENCH_FAKE_PAIR_TIMEOUT", "")      # test hook: "first" | "timed" exercise the two fall-backs
    if comm.max_float(float(eng.pair_timeouts() > 0 or fake_to == "first"), dev) != 0.0:
        eng.fused_pairs = False
        pairs_note = "switched off: a neighbour wait timed out in the first (untimed) steps"
        print(f"[bench] rank {comm.rank}: pair launches switched off (neighbour wait timed out in the first steps)", file=sys.stderr)
        step()
        torch.cuda.synchronize()

    # launch mode.  N = 1: the whole step is ONE hipGraph.  N > 1: the step is captured as hipGraph SEGMENTS cut at the
    # collectives (RCCL calls stay eager between two graph launches), so every rank replays the same kernels as the N = 1 run.
    graph, seg, launch = None, None, "eager"
    n_warm_eager = 0                         # (the two eager steps above; the W warm-up steps run in the timed launch mode)
    torch.cuda.synchronize()
    if not args.no_graph:
        try:
            if dcomm is None:
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    step()
                torch.cuda.current_stream().wait_stream(s)
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=s):
                    step()
                launch = "hipGraph"
            else:
                seg = eng.capture_train_step(xd, xd, cfg, lpc_x=lpcd, comm=dcomm)
                launch = f"hipGraph segments ({seg.nseg}) + {seg.ncoll} eager collective(s)"
        except Exception as ex:  # fall back to eager launches in this process, say so in the JSON
            print(f"[bench] hipGraph capture failed ({type(ex).__name__}: {ex}); running eagerly", file=sys.stderr)
            graph, seg, launch = None, None, f"eager (capture failed: {type(ex).__name__})"
    # First contact of the segmented replay with the real backend: one replay under try.  A rank whose replay throws (a
    # collective that refuses to run between graph launches, a graph that refuses to launch) says so, ALL ranks then agree
    # - through a collective of their own - to run eagerly in this process.  If the backend itself is broken that agreement
    # throws too and the rank exits non-zero: nothing is re-exec'ed or restarted once the GPU has been touched.
    if seg is not None:
        failed, why = 0.0, ""
        try:
            seg.replay()
            torch.cuda.synchronize()
        except Exception as ex:
            failed, why = 1.0, f"{type(ex).__name__}: {ex}"
            print(f"[bench] rank {comm.rank}: first segmented replay failed ({why}); asking all ranks to run eagerly", file=sys.stderr)
        if comm.max_float(failed, dev) != 0.0:
            seg = None
            launch = "eager (first segmented replay failed" + (f": {why.split(':')[0]}" if why else " on another rank") + ")"
            torch.cuda.synchronize()
            step()                           # the eager step must work, or the run ends here with its error
            torch.cuda.synchronize()
    run = graph.replay if graph is not None else (seg.replay if seg is not None else step)
    # every rank must take the same path (a rank that fell back to eager launches would still be correct, but say so)
    all_same = comm.max_float(0.0 if (graph is not None or seg is not None or args.no_graph) else 1.0, dev) == 0.0
    for _ in range(max(0, args.warmup - n_warm_eager)):
        run()
    torch.cuda.synchronize()

    pass_steps = pass_sizes(args.steps, args.passes)

    def timed_passes():
        ms = []
        for n in pass_steps:
            comm.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                run()
            torch.cuda.synchronize()
            comm.barrier()
            ms.append(1e3 * comm.max_float(time.perf_counter() - t0, dev) / n)
        return ms
    pass_ms = timed_passes()
    pair_to = eng.pair_timeouts()            # neighbour waits of the pair launches that timed out in ANY step so far (sticky counter): must be 0
    if comm.max_float(float(pair_to > 0 or fake_to == "timed"), dev) != 0.0:
        # a timed step ran with a neighbour wait that gave up (its results are invalid): all ranks drop the pair launches and the
        # captured graph, and the K steps are timed again with one eager launch per block - a slower line instead of none
        print(f"[bench] rank {comm.rank}: {pair_to} neighbour wait(s) of a pair launch timed out in the timed region; timing again "
              "with one launch per block, eagerly", file=sys.stderr)
        eng.fused_pairs = False
        pairs_note = "switched off after a neighbour wait timed out in the timed region; the K steps were timed again"
        graph, seg, run = None, None, step
        launch = "eager (pair launches switched off after a time-out; captured graph dropped)"
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        to_before = pair_to
        pass_ms = timed_passes()
        pair_to = eng.pair_timeouts() - to_before
        if pair_to:
            raise SystemExit(f"[bench] {pair_to} neighbour wait(s) timed out with pair launches off: results invalid")
    # what the last timed step computed, before anything below steps the engine again
    if args.dump_outputs and comm.rank == 0:
        done = dump_outputs(args.dump_outputs, step_outputs(eng, last_terms))
        sampled = [k for k, (_, whole) in done.items() if not whole]
        print(f"[bench] wrote {len(done)} arrays of the last timed step to {args.dump_outputs}"
              + (f" (sampled: {', '.join(sampled)})" if sampled else ""), file=sys.stderr)
    ms_step = float(np.median(pass_ms))
    dt = ms_step * 1e-3 * args.steps
    fps = comm.world * B * args.steps / dt

    # ---- the SAME step with the gated blocks on the exact fp32 matrix instruction, timed beside the headline (N = 1): what the
    # split-operand kernels buy, measured in the same run on the same parameters ----
    ms_exact = None
    if split_on and comm.world == 1 and dcomm is None and not args.no_graph:
        keep = (eng.split_fwd, eng.split_wgrad_arith, eng.split_dgrad, eng.split_conv)
        eng.split_fwd = eng.split_wgrad_arith = eng.split_dgrad = eng.split_conv = False
        try:
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            s2 = torch.cuda.Stream()
            s2.wait_stream(torch.cuda.current_stream())
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, stream=s2):
                step()
            for _ in range(3):
                g2.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                g2.replay()
            torch.cuda.synchronize()
            ms_exact = 1e3 * (time.perf_counter() - t0) / args.steps
            del g2
        except Exception as ex:
            print(f"[bench] exact-arm timing skipped ({type(ex).__name__}: {ex})", file=sys.stderr)
        eng.split_fwd, eng.split_wgrad_arith, eng.split_dgrad, eng.split_conv = keep
        step()
        torch.cuda.synchronize()

    # ---- roofline of the dominant kernel: per-launch HIP events on extra (eager) steps of the same workload ----
    # Kernels are timed IN ISOLATION: the side-stream overlap of the weight-gradient kernels is switched off for these
    # steps (otherwise a kernel's event bracket also contains whatever shares the CUs with it).
    ov = eng.overlap_wgrad
    eng.overlap_wgrad = False
    for _ in range(3):      # keep the stream busy so the instrumented launches below are queued behind real work:
        step()              # their events then time the GPU, not the host's launch latency
    eng.prof = []
    for _ in range(args.prof_steps):
        step()
    torch.cuda.synchronize()
    summ = eng.prof_summary()
    eng.prof = None
    eng.overlap_wgrad = ov
    # What an event bracket adds to the kernel inside it, measured live: an eager launch between two event records pays the
    # barrier packets of the records and a dispatch that cannot be queued behind its predecessor (the rocprofv3 kernel trace of
    # this same command shows the kernels ~5 us shorter than their brackets; inside the timed hipGraph they run back to back).
    # bracket(1 launch) = k + o, bracket(2 launches) = 2 k + o  ->  o = 2 t1 - t2, on nsc_spin (a dependent FMA chain: no cache can change its duration); the gap
    # between the two back-to-back launches counts as kernel time, so the estimate errs on the small side.
    brk_us, cal_us = 0.0, (0.0, 0.0)
    if summ:
        from nsc_amd import _lib as _l
        _lb = _l.load()
        sink = torch.zeros(4, device=dev)
        st_ = eng.stream()
        def _cal(nl):
            ts = []
            for _ in range(12):
                a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                step()                                   # (brackets queued behind real work, like the instrumented ones)
                a_.record()
                for _ in range(nl):
                    _l.check(_lb.nsc_spin(sink.data_ptr(), 20000, st_), "spin")
                b_.record()
                ts.append((a_, b_))
            torch.cuda.synchronize()
            return float(np.median([x.elapsed_time(y) for x, y in ts])) * 1e3
        t1, t2 = _cal(1), _cal(2)
        cal_us = (round(t1, 2), round(t2, 2))
        brk_us = float(min(max(2.0 * t1 - t2, 0.0), 10.0))
        summ = {tag: (n, max(ms - n * brk_us * 1e-3, 0.5 * ms), fl) for tag, (n, ms, fl) in summ.items()}
    # dominant kernel = the instrumented kernel class with the largest share of the step
    KERNELS = {"conv_mfma": "conv1d_fwd_kernel / conv1d_fwd_m32_kernel (convs outside gated blocks: forward + data gradients)",
               "block_fwd": ("gated_block_fwd3_pair_kernel / gated_block_fwd3_kernel (split operands on the bf16 matrix cores; persistent gated block forward, the two blocks of a stack per launch)"
                             if eng.split_fwd else
                             "gated_block_fwd2_pair_kernel / gated_block_fwd2_kernel (persistent weight-stationary gated block forward; the two blocks of a stack per launch)"),
               "block_wgrad": ("gated_block_wgrad_split_batch_kernel + slab_reduce_batch_kernel (split operands on the bf16 matrix cores; all blocks' weight gradients, one launch per width)"
                               if eng.split_wgrad_arith else
                               "gated_block_wgrad_batch_kernel + slab_reduce_batch_kernel (all blocks' weight gradients, one launch per width)"),
               "block_dgrad": "gated_block_dgrad2_pair_kernel / gated_block_dgrad2_kernel (persistent weight-stationary gated block data-path backward; the two blocks of a stack per launch)",
               "conv_split": "conv_split_kernel (the stride-2 down-sampling convs, forward + polyphase data gradient, split operands on the bf16 matrix cores)",
               "wgrad_mfma": "conv1d_wgrad_batch_kernel + conv_slab_reduce_batch_kernel (weight gradients of the convs outside gated blocks)"}
    roof, by_kernel = None, {}
    traffic = {}
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")   # bytes per launch from rocprofv3 --pmc FETCH_SIZE/WRITE_SIZE
    if os.path.exists(tpath):
        traffic = json.load(open(tpath))
    for tag, (n, ms, fl) in summ.items():
        ach = fl / (ms * 1e-3) / 1e12 if ms > 0 else 0.0
        by_kernel[tag] = dict(ms_per_step=round(ms / args.prof_steps, 3), launches_per_step=n // args.prof_steps,
                              achieved_tflops=round(ach, 2))
    mf = {k: v for k, v in summ.items() if k in KERNELS and k != "conv_split"}
    if mf:
        tag = max(mf, key=lambda k: mf[k][1])
        n, ms, fl = mf[tag]
        ach = fl / (ms * 1e-3) / 1e12
        roof = dict(bound="mfma", kernel=KERNELS[tag], achieved=round(ach, 3), peak=PEAK_F32_MFMA_TFLOPS, unit="TFLOP/s",
                    frac=round(ach / PEAK_F32_MFMA_TFLOPS, 4), traffic=traffic.get(tag),
                    launches_per_step=n // args.prof_steps, avg_launch_us=round(1e3 * ms / n, 2),
                    avg_launch_us_event_bracket=round(1e3 * ms / n + brk_us, 2), event_bracket_overhead_us=round(brk_us, 2), bracket_of_one_and_two_spin_launches_us=cal_us,
                    timing="HIP events around every launch of extra eager steps, minus the bracket's own overhead measured in the same "
                           "run (bracket of one vs two back-to-back launches of a cache-independent kernel); agrees with the rocprofv3 "
                           "kernel-trace average of this command (profiles/)",
                    flop_per_launch_avg=fl / n, peak_measured_on_box=153.7)
    kern_ms = by_kernel
    # the classes that run on split operands, priced against the bf16 matrix peak / 6 (six bf16 products per fp32-class product)
    roof_split = None
    if split_on:
        roof_split = {"peak": round(PEAK_SPLIT6_TFLOPS, 1), "unit": "TFLOP/s",
                      "peak_basis": "dense bf16 MFMA peak (2500 TFLOP/s, MI355X_MICROARCH.md) / 6: every fp32-class product is six bf16 products "
                                    "(three bf16 pieces per operand, fp32 accumulate); algorithmic FLOPs of the class / its time",
                      "classes": {}}
        for tag, on in (("block_fwd", eng.split_fwd), ("block_wgrad", eng.split_wgrad_arith), ("block_dgrad", eng.split_dgrad),
                        ("conv_split", eng.split_conv)):
            if on and tag in summ:
                n, ms, fl = summ[tag]
                ach = fl / (ms * 1e-3) / 1e12
                roof_split["classes"][tag] = dict(kernel=KERNELS[tag], achieved=round(ach, 2), frac=round(ach / PEAK_SPLIT6_TFLOPS, 4),
                                                  frac_of_f32_mfma_peak=round(ach / PEAK_F32_MFMA_TFLOPS, 4),
                                                  launches_per_step=n // args.prof_steps, avg_launch_us=round(1e3 * ms / n, 2))

    # HBM-bound quantizer at the op-surface form (p materialised, 34 816 B/frame fwd): measured at the config-5 batch
    qroof = None
    if comm.rank == 0 and args.config == 3:
        import ctypes as C
        from nsc_amd import _lib
        lib = _lib.load()
        Bq, L, nb = 4096, 256, 32
        code = torch.tanh(torch.randn(Bq, L, 1, device=dev))
        p = torch.empty(Bq, L, nb, device=dev); outq = torch.empty_like(code)
        qv = torch.empty(Bq, device=dev); hist = torch.zeros(nb, device=dev)
        c0 = eng.codecs[0]
        st = torch.cuda.current_stream().cuda_stream
        def qf():
            _lib.check(lib.nsc_quantize_fwd(code.data_ptr(), eng.p_ptr + 4 * c0.alpha_off, eng.p_ptr + 4 * c0.bins_off, 1.0, 1,
                                            Bq, L, nb, p.data_ptr(), outq.data_ptr(), qv.data_ptr(), hist.data_ptr(), st), "q")
        for _ in range(3):
            qf()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            qf()
        e1.record(); torch.cuda.synchronize()
        us = 1e3 * e0.elapsed_time(e1) / 20
        byts = Bq * L * (4 + 4 * nb + 4)
        # the launch the TRAINING step makes: fused-loss variant (p never written: 8 B per code), one launch per codec
        Bt = B
        ct = torch.tanh(torch.randn(Bt, L, 1, device=dev)); ot = torch.empty_like(ct)
        qt = torch.empty(Bt, device=dev)
        def qft():
            _lib.check(lib.nsc_quantize_fwd(ct.data_ptr(), eng.p_ptr + 4 * c0.alpha_off, eng.p_ptr + 4 * c0.bins_off, 1.0, 1,
                                            Bt, L, nb, None, ot.data_ptr(), qt.data_ptr(), hist.data_ptr(), st), "q")
        for _ in range(3):
            qft()
        e0.record()
        for _ in range(50):
            qft()
        e1.record(); torch.cuda.synchronize()
        ust = 1e3 * e0.elapsed_time(e1) / 50
        qtrain = dict(kernel=f"quantize_fwd_kernel (training shape: B={Bt}, p not materialised, 8 B/code)",
                      bytes_per_launch=Bt * L * 8, avg_launch_us=round(ust, 2), achieved_gbps=round(Bt * L * 8 / ust / 1e3, 1),
                      note="latency-bound: 262 KB per launch; the roofline record above is the op-surface form at the config-5 batch")
        qroof = dict(bound="hbm", kernel="quantize_fwd32_wave_kernel (one wave per frame; p materialised, B=4096 frames)", achieved=round(byts / us / 1e3, 1),
                     peak=8000.0, unit="GB/s", frac=round(byts / us / 1e3 / 8000.0, 4),
                     traffic=next((v for k, v in traffic.items() if k.startswith("quantize_fwd_wave@grid")), None), training_shape=qtrain,
                     bytes_per_launch=byts, avg_launch_us=round(us, 2), peak_measured_on_box=6800.0,
                     note="peak_measured_on_box = a write-only probe in the kernel's own grid and store geometry (probes library, tools/quant_time.py, profiles/r04a_quantizer_variants.txt): the kernel writes 32 of every 34 bytes; with its stores dropped the kernel's arithmetic alone takes 23.6 us (VALU-bound, not HBM-bound)")

    # ---- second half of the metric: codec forward us/frame (BASELINE config 5: 2-codec encode+quantise+decode,
    # batch 4096 frames, hipGraph-captured forward), plus the batch-1 latency the reference's eval loop actually pays
    infer = None
    if comm.rank == 0 and comm.world == 1 and not args.no_infer:
        def fwd_time(Bi, reps):
            engi = CascadeEngine(Bi, 2, BKD, [[2], [2]], [32, 32], res_scalar=RES_SCALAR, scale_first=True, lpc=True, device=dev)
            engi.set_params(eng.params)
            engi.refresh_wt()                    # once after loading weights: the forward takes the parameter-image prologue
            engi.keep_activations = False        # encode + quantise + decode only: nothing is kept for a backward pass
            xi = torch.from_numpy(np.tile(x_np, (max(1, Bi // B + 1), 1, 1))[:Bi].copy()).to(dev)
            for _ in range(2):
                engi.forward(xi, 1.0, False)
            torch.cuda.synchronize()
            gi = None
            try:
                si = torch.cuda.Stream()
                si.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(si):
                    engi.forward(xi, 1.0, False)
                torch.cuda.current_stream().wait_stream(si)
                gi = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gi, stream=si):
                    engi.forward(xi, 1.0, False)
            except Exception:
                gi = None
            runi = gi.replay if gi is not None else (lambda: engi.forward(xi, 1.0, False))
            runi(); torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(reps):
                runi()
            torch.cuda.synchronize()
            return (time.perf_counter() - t1) / reps, gi is not None
        tb, g1 = fwd_time(4096, 5)
        t1f, g2 = fwd_time(1, 50)
        infer = dict(batch=4096, us_per_frame=round(1e6 * tb / 4096, 3), ms_per_batch=round(1e3 * tb, 3),
                     frames_per_s=round(4096 / tb, 1), launch="hipGraph" if g1 else "eager",
                     batch1_latency_us=round(1e6 * t1f, 1), hard_codes=True,
                     tflops=round(4096 / tb * 476.1e6 / 1e12, 2))

    surface = None
    if comm.rank == 0 and comm.world == 1 and not args.no_op_surface and not args.no_infer:
        try:
            surface = op_surface_leg(B, x_np, dev)
        except Exception as e:                               # a side leg never takes the headline line down with it
            print(f"[bench] op_surface leg failed ({type(e).__name__}: {e})", file=sys.stderr)
            surface = dict(error=f"{type(e).__name__}: {e}")
            torch.cuda.synchronize()

    cpu = None
    if comm.rank == 0 and comm.world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(B, x_np, lpc_np)

    if comm.rank == 0:
        out = {
            "metric": "512-sample frames/s train step (2-codec CMRL)", "value": round(fps, 1), "unit": "frames/s",
            "n_gpus": comm.world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_step, 3), "ms_per_step_passes": [round(v, 3) for v in pass_ms],
            "ms_per_step_min": round(min(pass_ms), 3), "timing": f"median of {len(pass_ms)} passes ({' + '.join(map(str, pass_steps))} = {args.steps} steps), each bracketed by barrier + synchronize, max over ranks",
            "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("f32 (" + " + ".join(n_ for n_, on in (("gated-block forward", eng.split_fwd), ("gated-block weight gradients", eng.split_wgrad_arith),
                                                             ("gated-block data gradient", eng.split_dgrad),
                                                             ("stride-2 convs forward + data gradient", eng.split_conv)) if on) +
                      ": fp32 operands split into 3 bf16 pieces, 6 products on the bf16 matrix cores, fp32 accumulate - fp32-class error, "
                      "gate: tests/test_fullsize_gpu.py::_numerics_gate, profiles/r06_numerics_gate_*.txt; everything else: exact fp32)") if split_on else "f32",
            "data": "synthetic",
            "config": {"workload": (wl_name or "BASELINE config 3: 2-codec CMRL (strides [2], 32 bins) on fed LPC residual + 16x256 "
                                    "LSF quantizer, joint finetune step, fwd+loss+bwd+TF1-Adam") +
                                   ("+RCCL grad all-reduce(sum)" if comm.world > 1 else ""),
                       "batch_per_gpu": B, "global_batch": B * comm.world, "frame": 512,
                       **({"launch_note": os.environ["NSC_BENCH_LAUNCH_NOTE"]} if os.environ.get("NSC_BENCH_LAUNCH_NOTE") else {}),
                       "parallelism": f"dp{comm.world}", "block_arithmetic": "split" if split_on else "exact", "launch": launch, "all_ranks_same_launch": all_same,
                       "c_abi_calls_per_step": calls_per_step, "pair_launches": bool(eng.fused_pairs), "pair_launch_timeouts": pair_to, **({"pair_launches_note": pairs_note} if pairs_note else {}),
                       "grad_message": (("one per trainable scope, under the backward pass" if eng.dp_overlap else
                                         "one at the tail of the step") if dcomm is not None else None),
                       "streams": ("one; at the tail of the step the convs' batched weight gradients run on a second stream beside the gated blocks'"
                                   if eng.tail_overlap else "one (weight gradients batched at the tail of the step)"),
                       "roofline_note": "per-kernel numbers: HIP events around each launch on extra eager steps of the same workload"},
            "model_tflops": round(fps * mflop_frame * 1e6 / 1e12, 2), "mflop_per_frame": mflop_frame,
            "ms_per_step_exact_f32": (round(ms_exact, 3) if ms_exact is not None else None),
            "roofline": roof, "roofline_split_operand_classes": roof_split, "roofline_quantizer": qroof, "cpu_baseline": cpu,
            "codec_forward": infer, "op_surface": surface, "kernels": kern_ms,
        }
        print(json.dumps(out), flush=True)
    comm.barrier()
    comm.close()


if __name__ == "__main__":
    main()
