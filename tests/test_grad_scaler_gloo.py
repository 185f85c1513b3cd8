"""Dynamic loss scaling in a data-parallel run, on CPU: world_size-2 `gloo` processes, SIMT-emulator build of the kernels
(the layout of tests/test_distributed_gloo.py).

The gradient all-reduce SUMS, so an inf / nan produced on one rank reaches every rank's arena; the non-finite check runs after
the reduce (FusedSGDEMA.step(lr, scaler=...)), so all ranks skip together, halve their scales together and keep equal
parameters — with no collective beyond the gradient exchange itself, in fp32 and with the bf16 gradient exchange."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, emu_lib, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), SY_EMU_THREADS="4")
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import streamyolo_amd as sy
    from streamyolo_amd import _lib, train_engine
    from streamyolo_amd.amp import DeviceGradScaler
    from streamyolo_amd.optim import FusedSGDEMA
    from streamyolo_amd.train_engine import TrainStep
    from oracle import streamyolo_oracle as O
    from streamyolo_amd.utils.synth import synth_state_dict, synth_frames, synth_labels
    _lib.use_library(emu_lib)
    cfg = O.OracleConfig.named("nano")
    sd = synth_state_dict(O.param_shapes(cfg), seed=0)
    train_engine.TrainPlan.BUCKET_BYTES = 256 << 10              # several buckets: the reduce starts inside the backward walk
    train_engine.TrainPlan.FIRST_BUCKET_BYTES = 32 << 10
    x = synth_frames(1, 64, 96, seed=20 + rank)                  # every rank its own data, the same initial weights
    lab, sup = synth_labels(1, 64, 96, 8, num_gt=4, seed=30 + rank)
    res = {}
    for comm in ("fp32", "bf16"):
        m = sy.build_model("nano")
        m.load_state_dict(sd, strict=True)
        m.train().set_compute_dtype("fp32")
        st = TrainStep(m, world_size=world, process_group=dist, grad_comm_dtype=comm)
        scaler = DeviceGradScaler(init_scale=2.0 ** 10, growth_interval=1000)
        poison = [False]
        real = st._reduce_bucket

        def reduce_bucket(k, main, side, real=real, st=st, poison=poison):
            # rank 1's LOCAL gradients overflow: planted after its backward pass wrote the bucket, before the exchange
            if poison[0] and rank == 1 and k == len(st.plan.buckets) - 1:
                lo, hi, _ = st.plan.buckets[k]
                st.plan.arena[(lo + hi) // 2] = float("inf")
            return real(k, main, side)
        st._reduce_bucket = reduce_bucket
        opt, log = None, []
        for it in range(5):                                      # iteration 3 (a replayed tape, buckets reduced during backward) overflows
            poison[0] = it == 3
            st.step(x, (lab, sup), scaler=scaler)
            if opt is None:
                opt = FusedSGDEMA(m)
            before = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).clone()
            opt.step(1e-3, scaler=scaler)
            after = torch.cat([p.detach().reshape(-1) for p in m.parameters()])
            both = [torch.zeros_like(after) for _ in range(world)]
            dist.all_gather(both, after)
            c = scaler.counters()
            log.append({"scale": scaler.get_scale(), "taken": c["steps_taken"], "skipped": c["steps_skipped"],
                        "moved": not torch.equal(before, after), "ranks_equal": torch.equal(both[0], both[1]),
                        "finite": bool(torch.isfinite(after).all()), "overlapped": st.last_overlapped})
        res[comm] = log
    torch.save(res, os.path.join(out_dir, "rank%d.pt" % rank))
    dist.destroy_process_group()


def test_overflow_on_one_rank_skips_the_step_on_every_rank(tmp_path):
    import subprocess
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "streamyolo_amd", "csrc"), "-j8", "emu"], check=True)
    emu_lib = os.path.join(ROOT, "tests", "emu", "_build", "libstreamyolo_emu.so")
    mp.spawn(_worker, args=(2, _free_port(), emu_lib, str(tmp_path)), nprocs=2, join=True)
    for r in range(2):
        res = torch.load(os.path.join(str(tmp_path), "rank%d.pt" % r))
        for comm in ("fp32", "bf16"):
            log = res[comm]
            assert [e["skipped"] for e in log] == [0, 0, 0, 1, 1], (r, comm, log)
            assert [e["taken"] for e in log] == [1, 2, 3, 3, 4], (r, comm, log)
            assert [e["scale"] for e in log] == [1024.0, 1024.0, 1024.0, 512.0, 512.0], (r, comm, log)
            assert [e["moved"] for e in log] == [True, True, True, False, True], (r, comm, log)
            assert all(e["ranks_equal"] and e["finite"] for e in log), (r, comm, log)
            assert log[3]["overlapped"] > 0, "the poisoned step must be one whose buckets are reduced during backward"
