"""Gradient accumulation on several ranks: two freshly started processes share the one device of the test box and
all-reduce over gloo (the pattern of tests/test_optim_ddp_gpu.py).  Only the last micro-batch of a window issues
collectives, over grad_acc; the replicas stay bit-identical and follow ONE process stepping on the joint batch.  The
C-ABI reducer is driven on the loop-back communicator of tests/test_ddp_gpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 1e-3


def _setup(dev, batch, N):
    """tests/test_ddp_gpu.py's model and joint batch under plain SGD (no momentum, decay or clip: Adam would turn the
    rounding noise of the zero-gradient k_proj.bias elements into full steps, see tests/test_optim_ddp_gpu.py)."""
    from oracle import w2v2_oracle as O
    from w2v2_speaker_amd.config import W2V2Config, Wav2Vec2RegularisationConfig
    from w2v2_speaker_amd.engine import Plan
    from w2v2_speaker_amd.optim import OptimConfig
    from w2v2_speaker_amd.optim.schedule import Constant
    from w2v2_speaker_amd.params import ParamStore
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    st = ParamStore(W2V2Config.tiny(), dev, torch.float32, head="aam", num_speakers=10)
    st.init_weights(seed=3)
    reg = Wav2Vec2RegularisationConfig(attention_dropout=0.0, feat_proj_dropout=0.0, hidden_dropout=0.0, layerdrop=0.0,
                                       mask_time_prob=0.0)
    tr = SpeakerTrainer(st, Plan(st, batch, 4000, train=True, reg=reg), Constant(LR, 0.0), optimizer=OptimConfig("sgd"),
                        accumulate_grad_batches=N)
    wav, label = O.synth_batch(4, 4000, 10, seed=11)          # the joint batch; rank r takes rows 2r, 2r+1, one per micro-batch
    return st, tr, wav.to(dev), label.to(dev)


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    count = [0]
    real = dist.all_reduce

    def counted(*a, **k):
        count[0] += 1
        return real(*a, **k)
    dist.all_reduce = counted
    # the collectives of one N = 1 step, on a store of its own
    _, one, wav, label = _setup(dev, 1, 1)
    one.train_step(wav[rank:rank + 1], label[rank:rank + 1])
    per_step, count[0] = count[0], 0
    st, tr, wav, label = _setup(dev, 1, 2)
    counts = []
    for _ in range(2):
        for k in range(2):
            i = 2 * rank + k
            tr.train_step(wav[i:i + 1], label[i:i + 1])
            counts.append(count[0])
            count[0] = 0
    torch.cuda.synchronize()
    q.put((rank, st.flat[:st.n_train].cpu().numpy(), per_step, counts, tr.step))     # by value (no shared-memory handle)
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_times_two_micro_batches_match_the_joint_batch():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=300) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    dev = torch.device("cuda", 0)
    st, tr, wav, label = _setup(dev, 4, 1)
    fresh = st.flat[:st.n_train].cpu()
    for _ in range(2):
        tr.train_step(wav, label)
    torch.cuda.synchronize()
    ref = st.flat[:st.n_train].cpu()
    (_, p0, per0, c0, s0), (_, p1, per1, c1, s1) = res
    assert np.array_equal(p0, p1), "replicas diverged"
    assert s0 == s1 == 2
    # no collective on the non-final micro-batches (PL's no_sync), the collectives of an N = 1 step on the final ones
    assert per0 == per1 and per0 > 1, (per0, per1)
    assert c0 == c1 == [0, per0, 0, per0], (c0, c1, per0)
    moved = float((ref - fresh).norm())
    err = float((torch.from_numpy(p0) - ref).norm())
    print(f"2 ranks x N = 2 x B = 1 vs joint batch: |dp| = {moved:.3e}, |p - p_joint| = {err:.3e}, {per0} collectives per step")
    assert moved > 0 and err < 5e-4 * moved        # tests/test_ddp_gpu.py's bound for two ranks against the joint batch


def test_c_abi_reducer_reduces_the_arena_its_buffer_names():
    """CAbiBucketAllReducer on the loop-back communicator (world 2: SUM = x 2).  With ``buffer = grad_acc`` the slice that
    is reduced is grad_acc's and grad is left alone; with ``buffer = None`` it is grad's, as it always was.  Through the
    trainer: N = 2 on that reducer ends bit-identical to N = 2 with no reducer (x 2 and x 1/2 are exact in f32), and a
    reducer without the attribute is refused by name."""
    from w2v2_speaker_amd.comm import CAbiBucketAllReducer, RcclComm
    from w2v2_speaker_amd.trainer import SpeakerTrainer
    dev = torch.device("cuda", 0)
    comm = RcclComm.loopback(2, 0)
    st, _, wav, label = _setup(dev, 2, 1)
    red = CAbiBucketAllReducer(st, comm)
    assert red.buffer is None
    st.grad_acc = torch.full_like(st.grad, 5.0)
    st.grad.fill_(3.0)
    s, e = red.ranges["head"]
    assert e > s
    red.buffer = st.grad_acc
    red.bucket_ready("head")
    red.wait()
    torch.cuda.synchronize()
    assert bool((st.grad_acc[s:e] == 10.0).all()) and bool((st.grad_acc[e:] == 5.0).all()) and bool((st.grad == 3.0).all())
    red.buffer = None
    red.bucket_ready("head")
    red.wait()
    torch.cuda.synchronize()
    assert bool((st.grad[s:e] == 6.0).all()) and bool((st.grad[e:] == 3.0).all()) and bool((st.grad_acc[s:e] == 10.0).all())
    outs = []
    for use in (False, True):
        st, tr, wav, label = _setup(dev, 2, 2)
        if use:
            tr = SpeakerTrainer(st, tr.plan, tr.schedule, reducer=CAbiBucketAllReducer(st, comm), optimizer=tr.optimizer,
                                accumulate_grad_batches=2)
            assert tr.world == 2
        for _ in range(2):
            tr.train_step(wav[:2], label[:2])
            tr.train_step(wav[2:], label[2:])
        tr.train_step(wav[:2], label[:2])
        tr.flush()                                             # a partial window goes through every bucket as well
        torch.cuda.synchronize()
        assert tr.step == 3
        if use:
            assert tr.reducer.buffer is st.grad_acc
        outs.append(st.flat[:st.n_train].clone())
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])

    class Old:                                                 # a caller's reducer from before the attribute existed
        world, ranges = 2, red.ranges
    with pytest.raises(TypeError, match="buffer"):
        SpeakerTrainer(st, tr.plan, tr.schedule, reducer=Old(), accumulate_grad_batches=2)
    SpeakerTrainer(st, tr.plan, tr.schedule, reducer=Old())    # N = 1 asks nothing new of a reducer
    comm.destroy()
