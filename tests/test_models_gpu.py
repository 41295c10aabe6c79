"""GPU (-m gpu): product modules and whole models vs the reference's golden vectors / the oracle, plus
size-independent properties at BASELINE.json's full sizes."""
import numpy as np
import pytest
import torch

import model_cases as MC
from kernel_cases import assert_close
from improving_segmentation_with_selfsupervised_depth_amd import hipops as H

pytestmark = pytest.mark.gpu


def test_blocks(golden):
    MC.run_blocks("cuda", golden)


def test_monodepth_loss_vs_reference(golden):
    MC.run_loss_vs_reference("cuda", golden)


def test_monodepth_loss_multi_tile_strips(golden, monkeypatch):
    monkeypatch.setenv("SEGSDE_PHOTO_TILES", "2")
    MC.run_loss_vs_reference("cuda", golden)


def test_monodepth_loss_stereo_frame(golden):
    MC.run_loss_stereo_frame("cuda", golden)


def test_monodepth_loss_stereo_only(golden):
    MC.run_loss_stereo_only("cuda", golden)


def test_monodepth_loss_four_frames(golden):
    MC.run_loss_four_frames("cuda", golden)


@pytest.mark.parametrize("which", ["dd1", "dd2", "jsd1", "jsd2", "pad1", "pad2"])
def test_decoders(golden, which):
    MC.run_decoders("cuda", golden, (which,))


@pytest.mark.parametrize("which", ["r18", "r50dil", "r18x2"])
def test_encoder(golden, which):
    MC.run_encoder("cuda", golden, (which,))


@pytest.mark.parametrize("name", ["r18_mono", "r18_jsd"])
def test_full_model_vs_reference_vectors(golden, name):
    MC.run_full_model("cuda", golden, name)


@pytest.mark.parametrize("name,shape", [("r50_mono", (2, 64, 128)), ("r101_jsd", (2, 64, 128)), ("r101_pad", (2, 64, 128)),
                                        ("r50_mono", (3, 96, 160)), ("r101_jsd", (2, 96, 224))],
                         ids=["r50_mono", "r101_jsd", "r101_pad", "r50_mono_3x96x160", "r101_jsd_2x96x224"])
def test_big_models_vs_oracle(name, shape):
    """ResNet-50/101 (dilated layer4, ASPP) whole-model step at 64x128 (and two other sizes / batches) against the CPU
    oracle on identical weights"""
    from oracle import nets as N, photometric as P, segmix as S
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss
    from improving_segmentation_with_selfsupervised_depth_amd.loss.loss import cross_entropy2d
    import bench
    cfg = MC.contract_cfgs()["cfgs"][name]
    sd = N.build_state_dict(cfg, 19, seed=7, randomize_bn=True, zero_attention=False)
    model = get_model(cfg, 19)
    model.load_state_dict(sd, strict=True)
    model.cuda().train()
    MC.dropout_eval(model)
    B, Hh, W = shape
    inp = bench.synthetic_inputs(B, Hh, W, "cpu", 3)
    Kt = torch.tensor([[1.1 * W, 0, 0.5 * W, 0], [0, 1.1 * W, 0.5 * Hh, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    inp[("K", 0)] = Kt.unsqueeze(0).repeat(B, 1, 1)
    inp[("inv_K", 0)] = torch.linalg.pinv(Kt).unsqueeze(0).repeat(B, 1, 1)
    gen = torch.Generator().manual_seed(11)
    noise = {s: torch.randn(B, 2, Hh, W, generator=gen) for s in range(4)}
    # oracle in fp32 (the reference's arithmetic) and in fp64 (ground truth): the whole-model gradient is ill-conditioned
    # at the 1e-2 level for some parameters (BatchNorm over 64 samples, auto-mask argmin flips), so the product is
    # required to be as close to the truth as the reference's own fp32 evaluation is, not closer than that is possible
    def oracle(dtype):
        cast = lambda v: v.to(dtype) if v.is_floating_point() else v
        sdo = {k: (cast(v.clone()).requires_grad_(True) if v.is_floating_point() and "running" not in k else cast(v.clone()))
               for k, v in sd.items()}
        inp_t = {k: cast(v) for k, v in inp.items()}
        out_o = N.model_forward(sdo, cfg, inp_t, train=True, dropout=False)
        lo = P.MonodepthLossOracle(**bench.loss_cfg(B, Hh, W)["training"]["monodepth_loss"], batch_size=B)
        lo.generate_images_pred(inp_t, out_o)
        tot_o = lo.compute_losses(inp_t, out_o, tiebreak_noise={s: cast(n) for s, n in noise.items()})["loss"]
        if "semantics" in out_o:
            tot_o = tot_o + S.cross_entropy2d(out_o["semantics"], inp_t["lbl"])
        if "intermediate_semantics" in out_o:
            tot_o = tot_o + S.cross_entropy2d(out_o["intermediate_semantics"], inp_t["lbl"])
        tot_o.backward()
        return out_o, tot_o, {k: v.grad for k, v in sdo.items() if v.is_floating_point() and v.requires_grad}
    out_o, tot_o, g32 = oracle(torch.float32)
    out64, tot64, g64 = oracle(torch.float64)
    # product
    inp_d = {k: v.cuda() for k, v in inp.items()}
    out = model(inp_d)
    lp = get_monodepth_loss(bench.loss_cfg(B, Hh, W), True)
    lp.tiebreak_noise = noise
    lp.generate_images_pred(inp_d, out)
    tot = lp.compute_losses(inp_d, out)["loss"]
    if "semantics" in out:
        tot = tot + cross_entropy2d(out["semantics"], inp_d["lbl"])
    if "intermediate_semantics" in out:
        tot = tot + cross_entropy2d(out["intermediate_semantics"], inp_d["lbl"])
    tot.backward()
    # outputs of a 100-layer network with BatchNorm over 64 samples at its deepest stages: judged against the float64
    # evaluation -- 1e-3 of the output's scale, or three times the error the reference's own fp32 arithmetic makes
    def close_to_truth(key, what):
        t = out64[key].detach()
        e_prod = float((out[key].detach().double().cpu() - t).norm())
        e_ref = float((out_o[key].detach().double() - t).norm())
        assert e_prod <= max(3 * e_ref, 1e-3 * float(t.norm())), (what, e_prod, e_ref, float(t.norm()))
        return e_prod / float(t.norm()), e_ref / float(t.norm())
    for s in range(4):
        print("disp%d rel. error vs fp64: product %.2e, fp32 reference arithmetic %.2e" % ((s,) + close_to_truth(("disp", s), "disp%d" % s)))
    if "semantics" in out:
        print("semantics rel. error vs fp64: product %.2e, fp32 reference arithmetic %.2e" % close_to_truth("semantics", "semantics"))
    assert_close(tot, tot64, rtol=1e-3, what="total loss")
    import numpy as np
    e_prod, e_ref, presence = [], [], []
    for k, p in model.named_parameters():
        t = g64[k]
        if t is None or p.grad is None:
            if not (t is None and p.grad is None):
                presence.append(k)
            continue
        den = float(t.norm()) + 1e-12
        e_prod.append(float((p.grad.double().cpu() - t).norm()) / den)
        e_ref.append(float((g32[k].double() - t).norm()) / den)
    assert not presence, presence[:5]
    e_prod, e_ref = np.array(e_prod), np.array(e_ref)
    print("relative gradient error vs fp64 truth: product median %.2e max %.2e | fp32 reference arithmetic median %.2e max %.2e"
          % (np.median(e_prod), e_prod.max(), np.median(e_ref), e_ref.max()))
    assert np.median(e_prod) <= max(3 * np.median(e_ref), 1e-3), (np.median(e_prod), np.median(e_ref))
    assert e_prod.max() <= max(5 * e_ref.max(), 5e-2), (e_prod.max(), e_ref.max())


def test_full_size_conv_adjoint_identities():
    """<conv(x), dy> = <x, dgrad(dy)> = <w, wgrad(x, dy)> at the benchmark's largest decoder layer (512x1024)"""
    dev = "cuda"
    g = H.ConvGeom(64, 64, 3, 1, 1, 1, True, 0, True)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(2, 256, 512, 64, generator=gen).to(dev)
    w = (torch.randn(64, 64, 3, 3, generator=gen) * 0.05).to(dev)
    y = H.conv_forward(g, x, None, H.pack_weight(w), None)
    dy = torch.randn(y.shape, generator=gen).to(dev)
    dx, _ = H.conv_dgrad(g, dy, H.pack_weight(w, True), w, (512, 1024))
    dw = H.conv_wgrad(g, x, None, dy)
    a = float((y.double() * dy.double()).sum())
    b = float((x.double() * dx.double()).sum())
    c = float((w.double() * dw.double()).sum())
    assert abs(a - b) <= 1e-4 * abs(a) and abs(a - c) <= 1e-4 * abs(a), (a, b, c)
    # linearity in x
    y2 = H.conv_forward(g, 2.0 * x, None, H.pack_weight(w), None)
    assert_close(y2, 2.0 * y, rtol=1e-5, atol=1e-5, what="linearity")


def test_full_size_loss_properties():
    """512x1024: identical frames + identity pose => zero photometric error, full identity... (size independent)"""
    dev = "cuda"
    B, Hh, W = 2, 512, 1024
    gen = torch.Generator().manual_seed(0)
    img = torch.rand(B, 3, Hh, W, generator=gen).to(dev)
    K = torch.tensor([[1000.0, 0, 512, 0], [0, 1000.0, 256, 0], [0, 0, 1, 0], [0, 0, 0, 1]]).unsqueeze(0).repeat(B, 1, 1)
    T = torch.eye(4).unsqueeze(0).repeat(B, 1, 1).to(dev)
    disp = torch.rand(B, 1, Hh, W, generator=gen).to(dev)
    col, grid, depth = H.warp_forward(disp, torch.linalg.pinv(K).to(dev), K.to(dev), T, img, 0.1, 100, True, True)
    assert_close(col, img, rtol=1e-3, atol=2e-3, what="identity warp")   # sub-pixel rounding of the projection
    err = torch.empty(B, 1, Hh, W, device=dev)
    H.reprojection_error(img, img, False, err[:, 0])
    assert float(err.abs().max()) < 1e-6
    # BN: normalised output has zero mean / unit variance per channel at a full-size activation
    x = (torch.randn(2, 256, 512, 64, generator=gen) * 3 + 1).to(dev)
    mean, invstd = H.bn_stats(x, None, None, 0.1, 1e-5, update_running=False)
    y = H.bn_apply(x, mean, invstd, None, None)
    m = y.double().mean((0, 1, 2))
    v = y.double().var((0, 1, 2), unbiased=False)
    assert float(m.abs().max()) < 1e-4 and float((v - 1).abs().max()) < 1e-3
    # mix: all-ones mask is the identity, all-zeros mask rolls the batch (idempotence-style checks, bit exact)
    ones = torch.ones(B, Hh, W, dtype=torch.int64, device=dev)
    assert torch.equal(H.mix(ones, img), img)
    assert torch.equal(H.mix(torch.zeros_like(ones), img), torch.roll(img, -1, 0))


def test_depthmix_unlabeled_step_vs_oracle():
    """Trainer.train_step_segmentation_unlabeled (train.py:653-724) composed from the package's pieces -- teacher forward,
    depthcomp mask from the teacher's online disparity, DepthMix of image and teacher softmax, student forward, pseudo-label
    loss, backward, EMA teacher update -- against the same sequence in the CPU oracle on identical weights."""
    from oracle import nets as N, segmix as S, trainer as OT
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    from improving_segmentation_with_selfsupervised_depth_amd.loader import transformsgpu
    from improving_segmentation_with_selfsupervised_depth_amd import hipops as H, trainer as T
    import bench
    cfg = MC.contract_cfgs()["cfgs"]["r18_jsd"]
    sd_s = N.build_state_dict(cfg, 19, seed=21, randomize_bn=True, zero_attention=False)
    sd_t = N.build_state_dict(cfg, 19, seed=22, randomize_bn=True, zero_attention=False)
    B, Hh, W = 2, 64, 128
    inp = bench.synthetic_inputs(B, Hh, W, "cpu", 5)
    margin, ft, cw = 0.03, 0.0, 1.0

    # ---- oracle
    def grads_of(sd):
        return {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.clone())
                for k, v in sd.items()}
    with torch.no_grad():
        out_t = N.model_forward({k: v.clone() for k, v in sd_t.items()}, cfg, dict(inp), train=True, dropout=False, use_pose_net=False)
    soft_o = torch.softmax(out_t["semantics"], dim=1)
    depth_o = 1.0 / out_t[("disp", 0)]                      # online depth of the teacher (train.py:690-699: depth from disp)
    mask_o = S.depthcomp_mask(depth_o, margin, ft)
    img_o, _ = S.mix(mask_o.unsqueeze(1).float(), data=inp[("color_aug", 0, 0)])
    softm_o, _ = S.mix(mask_o.unsqueeze(1).float(), data=soft_o)
    sdo = grads_of(sd_s)
    inp2 = dict(inp); inp2[("color_aug", 0, 0)] = img_o
    out_s = N.model_forward(sdo, cfg, inp2, train=True, dropout=False, use_pose_net=False)
    L_o, lab_o = OT.calc_pseudo_label_loss(softm_o, out_s["semantics"], cw)
    L_o.backward()

    # ---- product
    student, teacher = get_model(cfg, 19), get_model(cfg, 19)
    student.load_state_dict(sd_s, strict=True); teacher.load_state_dict(sd_t, strict=True)
    student.cuda().train(); teacher.cuda().train()
    MC.dropout_eval(student); MC.dropout_eval(teacher)
    inp_d = {k: v.cuda() for k, v in inp.items()}
    teacher.use_pose_net = False
    with torch.no_grad():
        o_t = teacher(inp_d)
    soft = torch.softmax(o_t["semantics"].detach(), dim=1)
    depth = 1.0 / o_t[("disp", 0)]
    mask = H.depthcomp_mask(depth, margin, ft)
    assert_close(soft, soft_o, rtol=1e-3, atol=1e-5, what="teacher softmax")
    agree = float((mask.cpu() == mask_o).float().mean())
    assert agree > 0.995, agree                              # ties at the margin may flip on a handful of pixels
    mask = mask_o.cuda()                                     # continue from the oracle's mask: identical composites
    img, _ = transformsgpu.mix(mask.unsqueeze(1).float(), data=inp_d[("color_aug", 0, 0)])
    softm, _ = transformsgpu.mix(mask.unsqueeze(1).float(), data=soft)
    assert torch.equal(img.cpu(), img_o)
    inp_d2 = dict(inp_d); inp_d2[("color_aug", 0, 0)] = img
    student.use_pose_net = False
    o_s = student(inp_d2)
    assert_close(softm, softm_o, rtol=1e-3, atol=1e-5, what="mixed teacher distribution")
    _, lab_own = T.calc_pseudo_label_loss(softm, o_s["semantics"].detach(), cw)
    assert float((lab_own.cpu() == lab_o).float().mean()) > 0.99          # a near-tie of the teacher may flip a pixel's label
    # the loss / gradient comparison continues from the ORACLE's distribution (like the mask above): identical pseudo labels,
    # so that the vector criterion below measures arithmetic and not a handful of flipped labels
    L, lab = T.calc_pseudo_label_loss(softm_o.cuda(), o_s["semantics"], cw)
    assert torch.equal(lab.cpu(), lab_o)
    assert_close(L, L_o, rtol=1e-3, what="pseudo-label loss")
    L.backward()
    # vector criterion against the same student pass evaluated in float64 (identical mixed inputs / teacher distribution)
    cast = lambda v: v.double() if v.is_floating_point() else v
    sd64 = {k: (cast(v.clone()).requires_grad_(True) if v.is_floating_point() and "running" not in k else cast(v.clone()))
            for k, v in sd_s.items()}
    out64 = N.model_forward(sd64, cfg, {k: cast(v) for k, v in inp2.items()}, train=True, dropout=False, use_pose_net=False)
    L64, _ = OT.calc_pseudo_label_loss(softm_o.double(), out64["semantics"], cw)
    L64.backward()
    MC.gradients_vs_truth(list(student.named_parameters()), {k: v.grad for k, v in sdo.items() if v.is_floating_point() and v.requires_grad},
                          {k: v.grad for k, v in sd64.items() if v.is_floating_point() and v.requires_grad}, "DepthMix student pass")
    # EMA teacher update after the step (train.py:535-537)
    before = {k: v.detach().clone() for k, v in teacher.named_parameters()}
    T.update_ema_variables(teacher, student, 0.99, 10)
    a = np.float32(min(1 - 1 / 11, 0.99)); b = np.float32(1 - min(1 - 1 / 11, 0.99))
    sp = dict(student.named_parameters())
    for k, v in teacher.named_parameters():
        assert torch.equal(v.data, a * before[k] + b * sp[k].data), k


def test_reducer_around_real_model_nccl():
    """cfg4's exchange step on the GPU: a 1-rank nccl (RCCL) group around the real ResNet-18 joint model -- gradients
    through the bucketed all-reducer are bit-identical to the un-reduced run, dead disparity heads stay out of the
    buckets, multi-backward steps reduce once per bucket"""
    MC.run_reducer_real_model("cuda", "nccl")


@pytest.mark.parametrize("mix_use_gt", [False, True], ids=["softmax", "mix_use_gt"])
def test_unlabeled_step_function_vs_oracle(mix_use_gt):
    """cfg5's step function (trainer.train_step_segmentation_unlabeled) vs the oracle restatement of train.py:653-724, without
    and with mix_use_gt (train.py:667-672; on in exp-212, the block cfg5 is defined from)"""
    MC.run_unlabeled_step("cuda", mix_use_gt=mix_use_gt)


def test_validation_tail_vs_reference(golden):
    """predict_test_disp in eval mode -> generate_depth_test_pred -> stored 8-bit depth estimate
    (joint_segmentation_depth.py:72-75, monodepth_loss.py:54-62, depth_estimator.py:80-91) vs the reference's vectors"""
    from oracle import nets as N
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss
    from improving_segmentation_with_selfsupervised_depth_amd.loader import depth_estimator
    import bench
    g = golden("valtail")
    cfg = MC.contract_cfgs()["cfgs"]["r18_mono"]
    sd = N.build_state_dict(cfg, 19, seed=77, randomize_bn=True)
    if MC._sd_hash(sd) != str(g["sd_hash"]):
        pytest.skip("torch RNG stream differs from the build container")
    model = get_model(cfg, 19)
    model.load_state_dict(sd, strict=True)
    model.cuda().eval()
    B, _, Hh, W = g["in_color_0_0"].shape
    lo = get_monodepth_loss(bench.loss_cfg(B, Hh, W), is_train=False)
    u8, out = depth_estimator.estimate_depth_maps(model, lo, {("color", 0, 0): g["in_color_0_0"].cuda()})
    for s in range(4):
        assert_close(out[("disp", s)], g["disp_%d" % s], rtol=1e-3, atol=1e-5, what="test disp %d" % s)
        assert_close(out[("depth", 0, s)], g["depth_%d" % s], rtol=1e-3, atol=0, what="test depth %d" % s)
    # quantisation to 8 bits: a disparity that differs in the last fp32 bits may fall on the other side of an integer
    diff = (u8.cpu().int() - g["export_u8"].int()).abs()
    assert int(diff.max()) <= 1 and float((diff > 0).float().mean()) < 0.02, (int(diff.max()), float((diff > 0).float().mean()))


def test_pose_model_input_all_vs_reference(golden):
    """pose_model_input = "all": one 9-channel pose network for the three frames (joint_segmentation_depth.py:52-68)"""
    import json
    from oracle import nets as N
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    g = golden("poseall")
    cfg = json.loads(str(g["cfg_json"]))
    sd = N.build_state_dict(cfg, 19, seed=55, randomize_bn=True)
    if MC._sd_hash(sd) != str(g["sd_hash"]):
        pytest.skip("torch RNG stream differs from the build container")
    model = get_model(cfg, 19)
    model.load_state_dict(sd, strict=True)
    model.cuda().train()
    inputs = {}
    for f in (0, -1, 1):
        inputs[("color", f, 0)] = inputs[("color_aug", f, 0)] = g["in_color_%d" % f].cuda()
    out = model(inputs)
    assert_close(out[("cam_T_cam", 0, -1)], g["T_m1"], rtol=1e-3, atol=1e-5, what="T-1")
    assert_close(out[("cam_T_cam", 0, 1)], g["T_p1"], rtol=1e-3, atol=1e-5, what="T+1")
    assert_close(out[("axisangle", 0, 1)], g["axisangle"], rtol=1e-3, atol=1e-6, what="axisangle")
    assert_close(out[("translation", 0, -1)], g["translation"], rtol=1e-3, atol=1e-6, what="translation")
    loss = sum((out[("cam_T_cam", 0, f)] ** 2).sum() for f in (-1, 1)) + out[("axisangle", 0, 1)].sum()
    loss.backward()
    named = dict(model.named_parameters())
    assert_close(named["models.pose.net.3.weight"].grad, g["grad_pose_last"], rtol=1e-3,
                 atol=1e-3 * float(g["grad_pose_last"].abs().max()), what="pose head gradient")
    # The stem gradient passes 17 ReLUs.  Measured on this very fixture (kernel interpreter, bit-identical arithmetic):
    # every block-output gradient and every weight gradient from layer1.1 upwards agrees with the float64 oracle to 5e-6;
    # in layer1.0 ONE of 65 536 pre-activations of the block's final ReLU is +4.5e-7 in float64 -- the product's BatchNorm
    # rounds it to <= 0, torch's fp32 rounds it to > 0 -- and that single mask flip moves every gradient below it by
    # 1...3e-3 of its norm (all upstream gradients of this loss have the same tiny magnitude).  Hence a norm-wise bound of
    # 1e-2 here instead of an element-wise 1e-3; the kernels themselves are at 1e-6 (tests/test_kernels_gpu.py).
    got, want = named["models.pose_encoder.encoder.conv1.weight"].grad.double().cpu(), g["grad_pose_conv1"].double()
    assert tuple(got.shape) == tuple(want.shape) == (64, 9, 7, 7)
    rel = float((got - want).norm() / want.norm())
    assert rel <= 1e-2, rel


def test_convblock_dropout2d():
    MC.run_convblock_dropout2d("cuda")


def test_weight_pack_scope():
    MC.run_weight_pack_scope("cuda")


def test_aspp_fanout_gradient_fusion():
    MC.run_aspp_fanout("cuda")


def test_decoder_activation_backward_is_fused():
    MC.run_decoder_activation_fusion("cuda")


def test_bench_selfspawn_two_ranks_one_device():
    """The first real N>1 launch path, on the 1-GPU box: ``python bench.py --gpus 2`` re-executes itself under
    torch.distributed.run with two ranks (knobs: both on device 0, gloo instead of RCCL) -- rendezvous on 127.0.0.1, parameter
    broadcast, per-rank inputs and RNG streams, hook-driven bucketed all-reduce in index order, live-set agreement,
    max-over-ranks timing, ONE JSON line from rank 0 as the last line of stdout."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SEGSDE_BENCH_ONE_DEVICE="1", SEGSDE_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    cp = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--workload", "cfg1", "--steps", "2",
                         "--warmup", "1", "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert cp.returncode == 0, cp.stderr[-3000:]
    line = cp.stdout.strip().splitlines()[-1]
    res = json.loads(line)
    assert res["n_gpus"] == 2 and res["config"]["ranks"] == 2 and res["config"]["backend"] == "gloo"
    assert res["config"]["allreduce_launches"] > 0 and res["config"]["global_batch"] == 2 * res["config"]["per_gpu_batch"]
    assert res["value"] > 0 and res["steps"] == 2 and res["scaling"] == "weak"
    assert "hbm_kernels" in res and "roofline" in res
    # the N > 1 line explains itself
    c = res["comm"]
    for k in ("allreduce_ms_per_step", "exposed_comm_ms", "ms_per_step_without_allreduce", "allreduce_launches_per_step",
              "allreduce_mb_per_step", "buckets", "bucket_mb", "overlap", "per_rank_ms_per_step", "rccl_env"):
        assert k in c, k
    assert len(c["per_rank_ms_per_step"]) == 2 and all(x > 0 for x in c["per_rank_ms_per_step"])
    assert c["buckets"] >= 1 and c["allreduce_launches_per_step"] >= c["buckets"] and c["allreduce_mb_per_step"] > 10
    assert c["overlap"] is True and c["bucket_mb"] == 32.0
    # knobs + the payload-only mode
    cp = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--workload", "cfg1", "--steps", "2",
                         "--warmup", "1", "--no-cpu-baseline", "--bucket-mb", "8", "--no-overlap", "--allreduce-only"],
                        capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert cp.returncode == 0, cp.stderr[-3000:]
    only = json.loads(cp.stdout.strip().splitlines()[-1])
    assert only["unit"] == "ms" and only["value"] > 0 and only["n_gpus"] == 2 and only["bucket_mb"] == 8.0
    assert only["buckets"] > c["buckets"] and abs(only["payload_mb"] - c["allreduce_mb_per_step"]) < 1.0


def test_real_model_two_ranks_one_gpu():
    """cfg4's exchange step with the REAL model and two ranks: the ResNet-18 joint seg+depth model of this package on two
    gloo ranks (both on this box's GPU, the real HIP library), different inputs per rank, the reference's two backward() calls
    per step: broadcast makes the replicas identical, the hook-driven bucketed reducer leaves the mean of the two local
    gradients on both, dropout seeds differ between replicas (tests/test_ddp_gloo.py::_worker_real_model)."""
    import test_ddp_gloo as TD
    TD.run_real_model_two_ranks("cuda", 600)


def test_fusion_handoffs_are_counted():
    MC.run_fusion_diagnostics("cuda")


def test_hip_graph_replay_matches_eager_steps():
    """bench.py --hip-graph: one whole training step (forward, monodepth loss, backward, clip, optimiser) captured as a hipGraph and
    replayed must leave exactly the parameters the eager steps leave (same kernels, same order; dropout in eval mode and a
    fixed tie-break noise so that both runs are deterministic)."""
    import copy
    import bench
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    from improving_segmentation_with_selfsupervised_depth_amd.models import layers as L_
    from improving_segmentation_with_selfsupervised_depth_amd.models.layers import weight_pack_scope
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss
    B, Hh, W = 2, 64, 128
    dev = torch.device("cuda")
    torch.manual_seed(3)
    cfg = bench.model_cfg("cfg1", Hh, W)
    base = get_model(cfg, 19).to(dev).train()
    MC.dropout_eval(base)
    inputs = bench.synthetic_inputs(B, Hh, W, dev, 5, with_labels=False)
    gen = torch.Generator().manual_seed(9)
    noise = {s: torch.randn(B, 2, Hh, W, generator=gen).to(dev) for s in range(4)}

    def make():
        model = copy.deepcopy(base)
        opt = torch.optim.SGD(model.parameters(), lr=1e-2, momentum=0.9, fused=True)
        loss_obj = get_monodepth_loss(bench.loss_cfg(B, Hh, W), is_train=True)
        loss_obj.tiebreak_noise = noise

        def step():
            with weight_pack_scope(model):
                opt.zero_grad(set_to_none=True)
                out = model(inputs)
                loss_obj.generate_images_pred(inputs, out)
                total = loss_obj.compute_losses(inputs, out)["loss"]
                total.backward()
                torch.nn.utils.clip_grad_norm_(model.parameters(), 10.0)
                opt.step()
                return total
        return model, step

    m_e, step_e = make()
    for _ in range(4):
        loss_e = step_e()
    m_g, step_g = make()
    L_.GRAPH_SAFE_DROPOUT[0] = True
    try:
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            step_g()
            step_g()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loss_g = step_g()
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
    finally:
        L_.GRAPH_SAFE_DROPOUT[0] = False
    assert torch.isfinite(loss_g).all()
    assert_close(loss_g, loss_e, rtol=1e-6, atol=0, what="loss of the 4th step")
    worst = 0.0
    for (k, pe), (_, pg) in zip(m_e.named_parameters(), m_g.named_parameters()):
        d = float((pe - pg).abs().max())
        worst = max(worst, d / (float(pe.abs().max()) + 1e-30))
    assert worst <= 1e-6, worst


@pytest.mark.parametrize("defer", [True, False], ids=["deferred_trunk", "encoder_per_call"])
@pytest.mark.parametrize("scenario", ["joint", "depthmix"])
def test_train_step_replay_vs_reference_caller(scenario, defer):
    """VERDICT r3 item 5a.  tests/golden/trainstep.npz holds what the reference's OWN ``Trainer.train_step`` (imported from
    /root/reference/train.py by tests/golden/make_trainstep.py, reference modules underneath) left after each of two
    iterations: the returned losses, per-parameter gradient / update norms, parameter, BatchNorm and EMA checksums.  The same
    script runs the same train.py over this package's modules on the kernel interpreter (log:
    tests/golden/trainstep_package_run.json).  Here the package's mirror of the call sequence (``trainer.train_step``:
    five ``backward()`` calls, ``freeze_backbone_bn``, parameter groups over ``model.models``, clipping, EMA) replays it
    on the GPU -- with the encoder back-propagated once per forward (``defer``: functional.defer_trunk, the default of
    ``trainer.train_step`` for these configurations) and once per ``backward()`` call like the reference."""
    import numpy as np
    import trainstep_case as TC
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss, get_segmentation_loss_function
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    from conftest import GOLDEN
    import os
    ref = dict(np.load(os.path.join(GOLDEN, "trainstep.npz"), allow_pickle=False))
    from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
    cfg = TC.full_cfg(scenario)
    cfg["training"]["defer_trunk_backward"] = defer
    gate0 = (Fn.TrunkGateFn.trunk_backwards, Fn.TrunkGateFn.parked_passes)
    model = get_model(cfg["model"], TC.NCLS)
    model.load_state_dict(TC.state_dict(scenario), strict=True)
    TC.no_dropout(model)
    model.cuda()
    ema = None
    if cfg["training"]["unlabeled_segmentation"] is not None:
        ema = T.create_ema_model(model, cfg, TC.NCLS).cuda()
        TC.no_dropout(ema)
    groups = T.get_train_params(model, cfg)
    assert [len(list(g["params"])) for g in groups] == list(ref[scenario + "_param_group_sizes"])
    o = cfg["training"]["optimizer"]
    opt = torch.optim.SGD(T.get_train_params(model, cfg), lr=o["lr"], weight_decay=o["weight_decay"], momentum=o["momentum"])
    assert [g["lr"] for g in opt.param_groups] == list(ref[scenario + "_param_group_lrs"])
    loss_fn = get_segmentation_loss_function(cfg)
    mono = get_monodepth_loss(cfg, is_train=True)
    mono.tiebreak_noise = {s: n.cuda() for s, n in TC.noise().items()}
    out = {}
    for it in range(TC.ITERS):
        before = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
        unl = TC.batch(200 + it, labeled=False, onehot=True) if ema is not None else None
        losses = T.train_step(model, opt, TC.batch(100 + it), it, cfg, loss_fn, mono, ema_model=ema, unlabeled_inputs=unl)
        TC.record(out, scenario, it, losses, model, ema, before)
    TC.compare(out, ref, scenario)
    ran, parked = Fn.TrunkGateFn.trunk_backwards - gate0[0], Fn.TrunkGateFn.parked_passes - gate0[1]
    # joint: one forward with one gate (the encoder's), two calls.  depthmix: the PAD decoder adds a gate of its own where its two
    # halves meet -- three forwards per iteration (labeled: 2 calls, unmixed and mixed: 1 call each) x two gates
    want = {"joint": (TC.ITERS, TC.ITERS), "depthmix": (6 * TC.ITERS, 2 * TC.ITERS)}[scenario] if defer else (0, 0)
    assert (ran, parked) == want, (ran, parked, want)


def test_train_step_under_the_amp_protocol():
    """``amp: True`` (train.py:300,468-528; the dec6 configs): ``trainer.train_step`` keeps the reference's protocol -- autocast around
    the forward and the segmentation loss, every loss through ``GradScaler.scale``, ``unscale_`` before the clipping,
    ``scaler.step`` / ``update`` -- and the kernels compute in fp32 (functional.fp32_region).  Loss scaling by a power of two is
    exact and every backward kernel is linear in the incoming gradient, so two iterations must reproduce the records of the
    reference's own fp32 ``Trainer.train_step`` (tests/golden/trainstep.npz) exactly like the ``amp: False`` replay does -- and
    the scaler must have grown no ``found_inf``."""
    import numpy as np
    import os
    import trainstep_case as TC
    from conftest import GOLDEN
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss, get_segmentation_loss_function
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    scenario = "joint"
    ref = dict(np.load(os.path.join(GOLDEN, "trainstep.npz"), allow_pickle=False))
    cfg = TC.full_cfg(scenario)
    cfg["training"]["amp"] = True
    model = get_model(cfg["model"], TC.NCLS)
    model.load_state_dict(TC.state_dict(scenario), strict=True)
    TC.no_dropout(model)
    model.cuda()
    o = cfg["training"]["optimizer"]
    opt = torch.optim.SGD(T.get_train_params(model, cfg), lr=o["lr"], weight_decay=o["weight_decay"], momentum=o["momentum"])
    loss_fn = get_segmentation_loss_function(cfg)
    mono = get_monodepth_loss(cfg, is_train=True)
    mono.tiebreak_noise = {s: n.cuda() for s, n in TC.noise().items()}
    scaler = torch.amp.GradScaler("cuda", enabled=True)
    out = {}
    for it in range(TC.ITERS):
        before = {k: p.detach().cpu().clone() for k, p in model.named_parameters()}
        losses = T.train_step(model, opt, TC.batch(100 + it), it, cfg, loss_fn, mono, scaler=scaler)
        assert all(v.dtype == torch.float32 for v in losses.values() if v.is_floating_point())   # (absent losses are int zeros, train.py:460-464)
        TC.record(out, scenario, it, losses, model, None, before)
    TC.compare(out, ref, scenario)
    assert float(scaler.get_scale()) == 65536.0          # no overflow was seen: the scale never backed off


def test_train_step_amp_with_f16_operands():
    """``amp: True`` with the reference's reduced-precision arithmetic (functional.AMP_COMPUTE = "f16": the convolutions created
    under autocast round their operands to fp16 in the kernel -- v_mfma_f32_32x32x16_f16, fp32 accumulation -- in all three
    directions; BatchNorm, losses, optimizer fp32; GradScaler protocol of train.py:468-528).  Against the fp32 step on the same
    weights and batch: losses within 1 %, the parameter update points the same way (cosine > 0.98 over all parameters, > 0.8
    for every sub-model: BatchNorm over this test's two small images amplifies the operands' rounding in the encoder, 0.86
    measured), nothing overflowed (the loss scale did not back off), and the half-precision kernels really ran."""
    import trainstep_case as TC
    from improving_segmentation_with_selfsupervised_depth_amd import functional as Fn
    from improving_segmentation_with_selfsupervised_depth_amd import trainer as T
    from improving_segmentation_with_selfsupervised_depth_amd.loss import get_monodepth_loss, get_segmentation_loss_function
    from improving_segmentation_with_selfsupervised_depth_amd.models import get_model
    scenario = "joint"
    runs = {}
    for tag, amp, comp in (("f32", False, "f32"), ("f16", True, "f16")):
        cfg = TC.full_cfg(scenario)
        cfg["training"]["amp"] = amp
        model = get_model(cfg["model"], TC.NCLS)
        model.load_state_dict(TC.state_dict(scenario), strict=True)
        TC.no_dropout(model)
        model.cuda()
        o = cfg["training"]["optimizer"]
        opt = torch.optim.SGD(T.get_train_params(model, cfg), lr=o["lr"], weight_decay=o["weight_decay"], momentum=o["momentum"])
        mono = get_monodepth_loss(cfg, is_train=True)
        mono.tiebreak_noise = {s: n.cuda() for s, n in TC.noise().items()}
        before = {k: p.detach().clone() for k, p in model.named_parameters()}
        scaler = torch.amp.GradScaler("cuda", enabled=amp)
        old, Fn.AMP_COMPUTE[0] = Fn.AMP_COMPUTE[0], comp
        seen = []
        orig = H.conv_forward

        def spy(g, *a, **k):
            seen.append(g.compute)
            return orig(g, *a, **k)
        H.conv_forward = spy
        try:
            losses = T.train_step(model, opt, TC.batch(100), 0, cfg, get_segmentation_loss_function(cfg), mono, scaler=scaler)
        finally:
            Fn.AMP_COMPUTE[0], H.conv_forward = old, orig
        assert all(c == (1 if amp else 0) for c in seen) and seen, (tag, set(seen))
        if amp:
            assert float(scaler.get_scale()) == 65536.0
        runs[tag] = (losses, {k: (p.detach() - before[k]) for k, p in model.named_parameters()})
    l32, l16 = runs["f32"][0], runs["f16"][0]
    for k in ("mono_loss", "segmentation_loss", "total_loss"):
        a, b = float(l32[k]), float(l16[k])
        assert abs(a - b) <= 1e-2 * abs(a), (k, a, b)
    u32, u16 = runs["f32"][1], runs["f16"][1]

    def cos(keys):
        a = torch.cat([u32[k].flatten() for k in keys]).double()
        b = torch.cat([u16[k].flatten() for k in keys]).double()
        return float((a @ b) / (a.norm() * b.norm() + 1e-30))
    assert cos(list(u32)) > 0.98, cos(list(u32))
    for sub in ("models.encoder.", "models.depth.", "models.segmentation.", "models.pose_encoder.", "models.pose."):
        keys = [k for k in u32 if k.startswith(sub) and float(u32[k].abs().max()) > 0]
        if keys:
            assert cos(keys) > 0.8, (sub, cos(keys))


def test_skip_gradient_fanout():
    MC.run_skip_gradient_fanout("cuda")


@pytest.mark.gpu
def test_deferred_trunk_backward():
    MC.run_deferred_trunk_backward("cuda")
