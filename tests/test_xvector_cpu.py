"""The x-vector path, host side (no GPU needed): the float64 stage restatement of tests/xvector_cases.py against float64 torch
autograd over torch's own modules, the parameter names / shapes / count, the new C-ABI symbols, the length validation and
the module's constructor errors."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

import xvector_cases as K
from w2v2_speaker_amd import xvector as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTOGRAD_BOUND = 1e-10      # rel-L2, two float64 evaluations of one formula (profiles/ecapa_stage_parity.txt uses the same)

NEW_SYMBOLS = ["w2v2_stat_pool_fwd", "w2v2_stat_pool_fwd_len", "w2v2_stat_pool_bwd"]


class _TorchXVector(torch.nn.Module):
    """The model from torch's own modules, named so that its state dict has the keys of the restatement."""

    def __init__(self):
        super().__init__()
        fe, cin = torch.nn.Module(), K.MELS
        fe.blocks = torch.nn.ModuleList()
        for c, k, d in zip(K.CHANNELS, K.KERNEL_SIZES, K.DILATIONS):
            conv, norm = torch.nn.Module(), torch.nn.Module()
            conv.conv = torch.nn.Conv1d(cin, c, k, dilation=d, padding=d * (k - 1) // 2, padding_mode="reflect")
            norm.norm = torch.nn.BatchNorm1d(c, eps=K.BN_EPS, momentum=K.BN_MOMENTUM)
            fe.blocks.extend([conv, torch.nn.LeakyReLU(K.SLOPE), norm])
            cin = c
        lin = torch.nn.Module()
        lin.w = torch.nn.Linear(2 * cin, K.LIN)
        fe.blocks.extend([torch.nn.Identity(), lin])
        self.feature_extractor = fe
        cl = torch.nn.Module()
        cl.norm, cl.DNN, cl.out = torch.nn.Module(), torch.nn.Module(), torch.nn.Module()
        cl.norm.norm = torch.nn.BatchNorm1d(K.LIN, eps=K.BN_EPS, momentum=K.BN_MOMENTUM)
        cl.DNN.block_0 = torch.nn.Module()
        cl.DNN.block_0.linear, cl.DNN.block_0.norm = torch.nn.Module(), torch.nn.Module()
        cl.DNN.block_0.linear.w = torch.nn.Linear(K.LIN, K.LIN)
        cl.DNN.block_0.norm.norm = torch.nn.BatchNorm1d(K.LIN, eps=K.BN_EPS, momentum=K.BN_MOMENTUM)
        cl.out.w = torch.nn.Linear(K.LIN, K.SPEAKERS)
        self.classifier = cl

    def forward(self, feat, label):
        rec = {"a": [], "x": []}
        x = feat.transpose(1, 2)                                   # [B, C, T]
        b = self.feature_extractor.blocks
        for i in range(len(K.CHANNELS)):
            a = b[3 * i].conv(x)
            x = b[3 * i + 2].norm(b[3 * i + 1](a))
            rec["a"].append(a)
            rec["x"].append(x)
        std, mean = torch.std_mean(x, dim=2)
        rec["pooled"] = torch.cat([mean, std + K.POOL_EPS], 1)
        rec["emb"] = b[-1].w(rec["pooled"])
        cl, act = self.classifier, F.leaky_relu
        h1 = cl.norm.norm(act(rec["emb"], K.SLOPE))
        rec["z"] = cl.DNN.block_0.linear.w(h1)
        h2 = cl.DNN.block_0.norm.norm(act(rec["z"], K.SLOPE))
        rec["logits"] = cl.out.w(h2)
        rec["loss"] = F.cross_entropy(torch.log_softmax(rec["logits"], 1), label)   # the reference's CE of log-probabilities
        return rec


def test_restatement_forward_and_every_gradient_vs_float64_autograd():
    sd = K.make_state_dict(11)
    feat, label = K.inputs(12)
    net = _TorchXVector().double()
    missing, unexpected = net.load_state_dict({n: v.double() for n, v in sd.items()}, strict=False)
    assert not unexpected and all(m.split(".")[-1] in ("running_mean", "running_var", "num_batches_tracked") for m in missing)
    net.train()
    ref = net(feat.double(), label)
    ref["loss"].backward()
    rec = K.forward_ref(sd, feat, label)
    G = K.backward_ref(sd, rec)
    Bt = K.B * K.T
    worst = 0.0
    for i in range(len(K.CHANNELS)):
        for got, want in ((rec["a"][i], ref["a"][i]), (rec["x"][i + 1], ref["x"][i])):
            worst = max(worst, K.rel_l2(got, want.detach().transpose(1, 2).reshape(Bt, -1)))
    for n in ("pooled", "emb", "z", "logits", "loss"):
        worst = max(worst, K.rel_l2(rec[n], ref[n].detach()))
    print(f"xvector-cpu: forward, worst rel-L2 vs autograd modules {worst:.2e}")
    assert worst <= AUTOGRAD_BOUND
    params = dict(net.named_parameters())
    assert set(G) == set(params) == set(sd)
    for n, p in params.items():
        err = K.rel_l2(G[n], p.grad)
        worst = max(worst, err)
        assert err <= AUTOGRAD_BOUND, (n, err)
    print(f"xvector-cpu: {len(G)} gradients, worst rel-L2 vs autograd {worst:.2e}")
    # running statistics of torch's BatchNorm1d after the one training forward
    rm, rv = K.running_ref(torch.zeros(K.CHANNELS[0]), torch.ones(K.CHANNELS[0]), rec["bn"][0]["mu"], rec["bn"][0]["var"], Bt)
    bn0 = net.feature_extractor.blocks[2].norm
    assert K.rel_l2(rm, bn0.running_mean) <= AUTOGRAD_BOUND and K.rel_l2(rv, bn0.running_var) <= AUTOGRAD_BOUND


def test_leaky_relu_gradient_at_zero_is_the_slope():
    a = torch.tensor([[-1.0, 0.0, 2.0]], dtype=torch.float64, requires_grad=True)
    F.leaky_relu(a, K.SLOPE).sum().backward()
    assert torch.equal(a.grad, K.leaky_grad(a.detach())) and float(a.grad[0, 1]) == K.SLOPE


def test_pool_reference_over_lengths_is_the_utterance_alone():
    x = torch.randn(3, 9, 4, generator=torch.Generator().manual_seed(1))
    lens = [9, 8, 4]
    _, _, out = K.stat_pool_fwd_ref(x, lens)
    for b, n in enumerate(lens):
        assert torch.equal(out[b:b + 1], K.stat_pool_fwd_ref(x[b:b + 1, :n])[2])


def test_parameter_names_shapes_and_count():
    cfg = X.XVectorConfig()
    shapes = X.xvector_param_shapes(cfg, 5994)
    assert shapes == K.param_shapes(40, (512, 512, 512, 512, 1500), (5, 3, 3, 1, 1), 512, 5994)
    assert list(shapes) == list(K.param_shapes(40, (512, 512, 512, 512, 1500), (5, 3, 3, 1, 1), 512, 5994))
    assert shapes["feature_extractor.blocks.0.conv.weight"] == (512, 40, 5)
    assert shapes["feature_extractor.blocks.12.conv.weight"] == (1500, 512, 1)
    assert shapes["feature_extractor.blocks.14.norm.bias"] == (1500,)
    assert shapes["feature_extractor.blocks.16.w.weight"] == (512, 3000)
    assert shapes["classifier.out.w.weight"] == (5994, 512)
    count = sum(torch.Size(s).numel() for s in shapes.values())
    convs = 40 * 512 * 5 + 512 * 512 * 3 * 2 + 512 * 512 + 512 * 1500 + 4 * 512 + 1500
    norms = 2 * (4 * 512 + 1500) + 4 * 512
    linears = 3000 * 512 + 512 + 512 * 512 + 512 + 512 * 5994 + 5994
    assert count == convs + norms + linears == 7_592_190
    assert X.XVectorConfig.tiny() == X.XVectorConfig(K.MELS, K.LIN, K.CHANNELS, K.KERNEL_SIZES, K.DILATIONS)
    assert X.xvector_param_shapes(X.XVectorConfig.tiny(), K.SPEAKERS) == K.param_shapes()


def test_store_on_the_cpu_state_dict_round_trip_and_buffers():
    st = X.XVectorStore(X.XVectorConfig.tiny(), "cpu", num_speakers=K.SPEAKERS)
    sd = K.make_state_dict(5)
    st.load_state_dict(sd)
    out = st.state_dict()
    for n, v in sd.items():
        assert torch.equal(out[n], v), n
    for n in ("feature_extractor.blocks.14.norm.running_mean", "feature_extractor.blocks.14.norm.running_var",
              "classifier.norm.norm.running_mean", "classifier.DNN.block_0.norm.norm.running_var",
              "classifier.norm.norm.num_batches_tracked"):
        assert n in out, n
    assert out["feature_extractor.blocks.14.norm.running_var"].shape == (44,)     # 44 channels everywhere, no padding
    assert st.g("feature_extractor.blocks.12.conv.weight").shape == (44, 16, 1)
    with pytest.raises(NotImplementedError):
        X.XVectorStore(X.XVectorConfig.tiny(), "cpu", torch.bfloat16, num_speakers=K.SPEAKERS)


def _c_type(t: str):
    t = t.strip()
    if "*" in t:
        return ctypes.c_void_p
    return {"int": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}[t.replace("const ", "")]


def test_new_symbols_declared_exported_and_wrapped_with_matching_signatures():
    hdr = open(os.path.join(ROOT, "include", "w2v2_hip.h")).read()
    src = open(os.path.join(ROOT, "w2v2_speaker_amd", "csrc", "tdnn.hip")).read()
    from w2v2_speaker_amd import _build, _lib, ops
    assert "tdnn.hip" in _build.SOURCES
    for name in NEW_SYMBOLS:
        m = re.search(r"int %s\(([^)]*)\);" % name, hdr)
        assert m, name
        assert name in _lib._SIGS and name in _lib.EXPORTS, name
        res, args = _lib._SIGS[name]
        declared = [_c_type(a.rsplit(" ", 1)[0] if "*" not in a else a) for a in m.group(1).replace("\n", " ").split(",")]
        assert res is ctypes.c_int32 and list(args) == declared, (name, args, declared)
        d = re.search(r'extern "C" int %s\(([^)]*)\)' % name, src)
        assert d and re.sub(r"\s+", " ", d.group(1)) == re.sub(r"\s+", " ", m.group(1)), name
    for name in ("W2V2_BN_ACT_NONE 0", "W2V2_BN_ACT_RELU 1", "W2V2_BN_ACT_LEAKY 2"):
        assert "#define " + name in hdr
    assert (ops.BN_ACT_NONE, ops.BN_ACT_RELU, ops.BN_ACT_LEAKY) == (0, 1, 2) == (int(False), int(True), 2)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    for fn in ("stat_pool_fwd", "stat_pool_bwd"):
        assert callable(getattr(ops, fn)), fn


def test_length_validation():
    from w2v2_speaker_amd.ecapa import valid_frame_lengths, valid_sample_lengths
    cfg = X.XVectorConfig()
    assert X.xvector_min_frames(cfg) == 4 == X.xvector_min_frames(X.XVectorConfig.tiny())     # k = 3, dilation 3: pad 3
    F.pad(torch.zeros(1, 1, 4), (3, 3), mode="reflect")                                   # torch's own rule: pad < length
    with pytest.raises(RuntimeError):
        F.pad(torch.zeros(1, 1, 3), (3, 3), mode="reflect")
    assert valid_frame_lengths(cfg, [100, 57, 4], 3, 100) == [100, 57, 4]
    with pytest.raises(ValueError):
        valid_frame_lengths(cfg, [100, 57, 3], 3, 100)
    with pytest.raises(ValueError):
        valid_frame_lengths(cfg, [101, 57, 4], 3, 100)
    with pytest.raises(ValueError):
        valid_frame_lengths(cfg, [100, 57], 3, 100)
    assert valid_sample_lengths(cfg, [480], 1, 480) == [480]                                # 1 + 480 // 160 = 4 frames
    with pytest.raises(ValueError):
        valid_sample_lengths(cfg, [479], 1, 480)


def test_module_constructor_errors_and_surface():
    from w2v2_speaker_amd.lightning_modules.speaker import XVectorModule, XVectorModuleConfig
    from w2v2_speaker_amd.lightning_modules.speaker._optim_surface import EmbeddingEvaluation, OptimizerSurface
    from w2v2_speaker_amd.optim.loss import AngularAdditiveMarginSoftMaxLoss, CrossEntropyLoss, TripletCrossEntropyLoss
    from w2v2_speaker_amd.optim import fused
    assert issubclass(XVectorModule, OptimizerSurface) and issubclass(XVectorModule, EmbeddingEvaluation)
    assert issubclass(X.XVectorTrainer, fused.WindowedTrainer)
    cfg = XVectorModuleConfig()
    assert (cfg.tdnn_blocks, cfg.tdnn_channels, cfg.tdnn_kernel_sizes, cfg.tdnn_dilations, cfg.lin_neurons, cfg.in_channels,
            cfg.explicit_stat_pool_embedding_size, cfg.explicit_num_speakers) == \
        (5, [512, 512, 512, 512, 1500], [5, 3, 3, 1, 1], [1, 2, 3, 1, 1], 512, 40, None, None)
    aam = lambda: AngularAdditiveMarginSoftMaxLoss(2, 2, device="cpu", act_dtype=torch.float32)
    with pytest.raises(ValueError, match="xvector does not support aam softmax"):
        XVectorModule(None, cfg, 7, aam, [], [], None, device="cpu")
    with pytest.raises(NotImplementedError):
        XVectorModule(None, cfg, 7, TripletCrossEntropyLoss, [], [], None, device="cpu")
    with pytest.raises(NotImplementedError):
        XVectorModule(None, cfg, 7, CrossEntropyLoss, [], [], None, device="cpu", act_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        XVectorModule(None, cfg, 7, CrossEntropyLoss, [], [], None, device="cpu", input_features="mfcc")
    for m in ("generate_example_input", "compute_speaker_embedding", "compute_speaker_prediction",
              "compute_speaker_embeddings", "evaluate_trials", "training_step", "set_optimizer", "from_config"):
        assert callable(getattr(XVectorModule, m)), m
