"""Data-parallel steps under Adam with weight decay and a gradient-norm clip that engages: two processes share the one
device of the test box and all-reduce over gloo (the pattern of tests/test_ddp_gpu.py; each process is started fresh).
After the all-reduce both replicas hold identical gradients; the fixed-order norm must give them an identical clip
coefficient, so they stay bit-identical, and they follow ONE process stepping on the joint batch."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# The gradient norm of this batch at these weights is ~70 over the three steps.  The clip sits at half of it (as in the
# single-step test of tests/test_optim_trainer_gpu.py), so it engages on every step.
CLIP = 35.0
WD = 1e-2

def _setup(dev, batch):
    from oracle import w2v2_oracle as O
    from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim import OptimConfig
    from w2v2_speaker_amd.optim.schedule import OneCycle
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    st = ParamStore(W2V2Config.tiny(), dev, torch.float32, head="aam", num_speakers=10)
    st.init_weights(seed=3)
    reg = Wav2Vec2RegularisationConfig(attention_dropout=0.0, feat_proj_dropout=0.0, hidden_dropout=0.0, layerdrop=0.0,
                                       mask_time_prob=0.0)
    plan = Plan(st, batch, 4000, train=True, reg=reg)
    wav, label = O.synth_batch(4, 4000, 10, seed=11)          # the joint batch; rank r takes rows 2r, 2r+1
    tr = SpeakerTrainer(st, plan, OneCycle(max_lr=1e-3, total_steps=10), optimizer=OptimConfig("adam", weight_decay=WD),
                        gradient_clip_val=CLIP)
    return st, tr, wav.to(dev), label.to(dev)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    st, tr, wav, label = _setup(dev, 2)
    coefs = []
    for _ in range(3):
        tr.train_step(wav[2 * rank:2 * rank + 2], label[2 * rank:2 * rank + 2])
        torch.cuda.synchronize()
        coefs.append(st.grad_norm.cpu().numpy().copy())
    q.put((rank, st.flat[:st.n_train].cpu().numpy(), np.stack(coefs)))     # by value (no shared-memory handle)
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_clipped_decayed_adam_stays_identical_and_matches_joint_batch():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    dev = torch.device("cuda", 0)
    st, tr, wav, label = _setup(dev, 4)
    fresh = st.flat[:st.n_train].cpu()
    for _ in range(3):
        tr.train_step(wav, label)
    torch.cuda.synchronize()
    ref = st.flat[:st.n_train].cpu()
    (_, p0, c0), (_, p1, c1) = res
    assert np.array_equal(p0, p1), "replicas diverged"
    assert np.array_equal(c0, c1), "the replicas computed different norms / clip coefficients"
    # attention.k_proj.bias has an identically zero gradient (softmax does not see a shift of every key's score by the
    # same amount), so what backward leaves there is rounding noise of ~1e-9, different for every summation order.
    # Plain Adam damps it (noise << eps).  With L2 decay the first noise step makes p non-zero, wd * p then IS the
    # gradient, and Adam's normalisation turns it into full-size steps whose sign the noise chose: two ranks and the
    # joint batch disagree there by the step length itself (measured: 2.6e-3 of the 2.6e-3 total difference sits in
    # these 128 elements, every other tensor agrees to 1.4e-7 or better; torch's own DDP would do the same).  Those
    # elements are held to what can be asked of them -- identical on both replicas (above), and no further from the
    # joint run than Adam can move an element, lr * (1 - beta1) / sqrt(1 - beta2) <= 3.2 lr per step -- and everything
    # else to the bound of tests/test_ddp_gpu.py.
    noise = torch.zeros(st.n_train, dtype=torch.bool)
    for name, off in st.offsets.items():
        if name.endswith("attention.k_proj.bias"):
            noise[off:off + st.shapes[name][0]] = True
    assert int(noise.sum()) == st.cfg.num_hidden_layers * st.cfg.hidden_size
    diff = torch.from_numpy(p0) - ref
    moved = float((ref - fresh)[~noise].norm())
    err = float(diff[~noise].norm())
    print(f"two-rank vs joint batch: |dp| = {moved:.3e}, |p_ddp - p_joint| = {err:.3e} (k_proj.bias: {float(diff[noise].norm()):.3e}), "
          f"coefficients {c0[:, 1]}")
    assert (c0[:, 1] < 1.0).all(), c0                          # the clip engaged on every step
    assert moved > 0 and err < 5e-4 * moved        # tests/test_ddp_gpu.py's bound: Adam normalises the update
    assert float(diff[noise].abs().max()) <= 2 * 3.2 * sum(tr.schedule.at(i)[0] for i in range(3))
