"""ORACLE tooling -- generates tests/golden/*.npz by IMPORTING the reference.

Runs only in the build container (needs /root/reference); the GPU box never
runs it.  Nothing from the reference is copied: only numbers (inputs/outputs)
are written.  Three shims are applied from outside:

1. ``torch.Tensor.cuda`` -> identity (hard-coded ``.cuda()`` at
   models/IRR_PWC.py:68-71, models/pwc_modules.py:111,129).
2. train mode only: ``rescale_flow`` replaced by an alias-preserving,
   autograd-legal equivalent (in-place ``mul_`` on the argument, returns a
   clone) -- the as-is function raises under modern autograd.
3. robust-mask mode: ``WarpingLayer.forward`` twin with threshold 0.9999.

Usage:  python oracle/gen_golden.py  [--out tests/golden]
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as tf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
REF = "/root/reference"
sys.path.insert(0, REF)

torch.Tensor.cuda = lambda self, *a, **k: self          # shim 1

import models  # noqa: E402  (reference package)
import losses  # noqa: E402
import irr_pwc_oracle as O  # noqa: E402

ref_irr = sys.modules["models.IRR_PWC"]
ref_pwc = sys.modules["models.pwc_modules"]
ref_irrm = sys.modules["models.irr_modules"]
_orig_rescale = ref_irr.rescale_flow
_orig_warp_forward = ref_pwc.WarpingLayer.forward


def _rescale_alias(flow, div_flow, width_im, height_im, to_local=True):   # shim 2
    if to_local:
        u = float(flow.size(3) / width_im / div_flow)
        v = float(flow.size(2) / height_im / div_flow)
    else:
        u = float(width_im * div_flow / flow.size(3))
        v = float(height_im * div_flow / flow.size(2))
    flow.mul_(torch.tensor([u, v]).view(1, 2, 1, 1))
    return flow.clone()


def _make_warp_forward(thr):                                               # shim 3
    def fwd(self, x, flow, height_im, width_im, div_flow):
        flo_w = flow[:, 0] * 2 / max(width_im - 1, 1) / div_flow
        flo_h = flow[:, 1] * 2 / max(height_im - 1, 1) / div_flow
        grid = torch.add(ref_pwc.get_grid(x), torch.stack([flo_w, flo_h]).transpose(0, 1))
        grid = grid.transpose(1, 2).transpose(2, 3)
        xw = tf.grid_sample(x, grid, align_corners=True)
        m = tf.grid_sample(torch.ones(x.size()), grid, align_corners=True)
        return xw * (m >= thr).float()
    return fwd


def set_mode(train_patch: bool, robust: bool):
    ref_irr.rescale_flow = _rescale_alias if train_patch else _orig_rescale
    ref_pwc.WarpingLayer.forward = _make_warp_forward(0.9999) if robust else _orig_warp_forward


def ref_model(params=None, seed=None):
    args = types.SimpleNamespace(batch_size=2, model_div_flow=0.05)
    if seed is not None:
        torch.manual_seed(seed)
    m = models.IRR_PWC(args)
    if params is not None:
        missing = m.load_state_dict(params, strict=True)
        assert not missing.missing_keys and not missing.unexpected_keys
    return m, args


def npf(t):
    return t.detach().cpu().numpy().astype(np.float32)


# ---------------------------------------------------------------- per-op fixtures
def gen_ops(out_dir):
    set_mode(False, False)
    g = torch.Generator().manual_seed(77)
    d = {}
    # cost volume: fwd + grads (reference Python path actually used by the model)
    for name, (b, c, h, w) in {"a": (2, 8, 12, 14), "b": (1, 32, 24, 28), "c": (1, 196, 6, 7),
                               "d": (2, 5, 9, 33)}.items():
        f1 = torch.randn(b, c, h, w, generator=g, requires_grad=True)
        f2 = torch.randn(b, c, h, w, generator=g, requires_grad=True)
        go = torch.randn(b, 81, h, w, generator=g)
        o = ref_pwc.compute_cost_volume(f1, f2, {"max_disp": 4})
        o.backward(go)
        d.update({f"corr_{name}_f1": npf(f1), f"corr_{name}_f2": npf(f2), f"corr_{name}_go": npf(go),
                  f"corr_{name}_out": npf(o), f"corr_{name}_g1": npf(f1.grad), f"corr_{name}_g2": npf(f2.grad)})
    # warp: out, mask bits, grads.  Flow magnitudes chosen so many samples leave the frame.
    wl = ref_pwc.WarpingLayer()
    for name, (b, c, h, w, H, W, amp) in {"a": (2, 3, 16, 24, 64, 96, 0.5), "b": (1, 32, 12, 14, 384, 448, 0.08),
                                          "c": (2, 2, 10, 17, 40, 68, 0.3), "z": (1, 4, 8, 8, 64, 64, 0.0)}.items():
        for thr_name, robust in (("asis", False), ("robust", True)):
            set_mode(False, robust)
            gg = torch.Generator().manual_seed(ord(name[0]) + 5)
            x = torch.randn(b, c, h, w, generator=gg, requires_grad=True)
            fl = (torch.randn(b, 2, h, w, generator=gg) * amp).requires_grad_(True)
            go = torch.randn(b, c, h, w, generator=gg)
            o = wl(x, fl, H, W, 0.05)
            o.backward(go)
            # mask bits as the reference computes them
            with torch.no_grad():
                ones = wl(torch.ones(b, 1, h, w), fl, H, W, 0.05)
            key = f"warp_{name}_{thr_name}"
            d.update({key + "_x": npf(x), key + "_flow": npf(fl), key + "_go": npf(go), key + "_out": npf(o),
                      key + "_mask": npf(ones), key + "_gx": npf(x.grad), key + "_gflow": npf(fl.grad),
                      key + "_HW": np.array([H, W], np.int64)})
    set_mode(False, False)
    # bilinear align_corners resize (up and down), fwd + grad
    for name, (b, c, h, w, oh, ow) in {"up": (2, 2, 6, 7, 12, 14), "down": (1, 3, 64, 96, 8, 12),
                                       "odd": (1, 1, 5, 9, 11, 13)}.items():
        x = torch.randn(b, c, h, w, generator=g, requires_grad=True)
        go = torch.randn(b, c, oh, ow, generator=g)
        o = tf.interpolate(x, [oh, ow], mode="bilinear", align_corners=True)
        o.backward(go)
        d.update({f"resize_{name}_x": npf(x), f"resize_{name}_go": npf(go), f"resize_{name}_out": npf(o),
                  f"resize_{name}_gx": npf(x.grad)})
    np.savez_compressed(os.path.join(out_dir, "ops_basic.npz"), **d)

    # module-level fixtures with synthetic weights (refine heads, occ upsampler, dense, context)
    P = O.synthetic_params(0)
    m, _ = ref_model(P)
    m.eval()
    d = {}
    b, h, w = 2, 12, 14
    flow = torch.randn(b, 2, h, w, generator=g, requires_grad=True)
    dimg = torch.randn(b, 3, h, w, generator=g, requires_grad=True)
    feat = torch.randn(b, 32, h, w, generator=g, requires_grad=True)
    go = torch.randn(b, 2, h, w, generator=g)
    o = m.refine_flow(flow, dimg, feat)
    o.backward(go)
    d.update(rf_flow=npf(flow), rf_dimg=npf(dimg), rf_feat=npf(feat), rf_go=npf(go), rf_out=npf(o),
             rf_gflow=npf(flow.grad), rf_gdimg=npf(dimg.grad), rf_gfeat=npf(feat.grad))
    occ = torch.randn(b, 1, h, w, generator=g, requires_grad=True)
    f1 = torch.randn(b, 32, h, w, generator=g, requires_grad=True)
    f2 = torch.randn(b, 32, h, w, generator=g, requires_grad=True)
    go = torch.randn(b, 1, h, w, generator=g)
    o = m.refine_occ(occ, f1, f2)
    o.backward(go)
    d.update(ro_occ=npf(occ), ro_f1=npf(f1), ro_f2=npf(f2), ro_go=npf(go), ro_out=npf(o),
             ro_gocc=npf(occ.grad), ro_gf1=npf(f1.grad), ro_gf2=npf(f2.grad))
    occ = torch.randn(b, 1, h, w, generator=g, requires_grad=True)
    guide = torch.randn(b, 10, 2 * h, 2 * w, generator=g, requires_grad=True)
    go = torch.randn(b, 1, 2 * h, 2 * w, generator=g)
    o = m.occ_shuffle_upsample(occ, guide)
    o.backward(go)
    d.update(ou_occ=npf(occ), ou_guide=npf(guide), ou_go=npf(go), ou_out=npf(o),
             ou_gocc=npf(occ.grad), ou_gguide=npf(guide.grad))
    x = torch.randn(1, 115, h, w, generator=g, requires_grad=True)
    xi, fo = m.flow_estimators(x)
    gi = torch.randn(xi.shape, generator=g)
    gf = torch.randn(fo.shape, generator=g)
    (xi * gi).sum().add((fo * gf).sum()).backward()
    d.update(de_x=npf(x), de_gi=npf(gi), de_gf=npf(gf), de_xi=npf(xi), de_out=npf(fo), de_gx=npf(x.grad))
    m.zero_grad()
    x = torch.randn(1, 565, 20, 24, generator=g, requires_grad=True)
    o = m.context_networks(x)
    go = torch.randn(o.shape, generator=g)
    o.backward(go)
    d.update(cn_x=npf(x), cn_go=npf(go), cn_out=npf(o), cn_gx=npf(x.grad),
             cn_gw0=npf(m.context_networks.convs[0][0].weight.grad)[:, :8],
             cn_gb0=npf(m.context_networks.convs[0][0].bias.grad),
             cn_gw4=npf(m.context_networks.convs[4][0].weight.grad)[:8],
             cn_gw6=npf(m.context_networks.convs[6][0].weight.grad))
    np.savez_compressed(os.path.join(out_dir, "ops_modules.npz"), **d)


# ---------------------------------------------------------------- end-to-end fixtures
def _flat_stats(out):
    st = []
    for key in ("flow", "occ"):
        for lvl in out[key]:
            for t in lvl:
                st.append([float(t.mean()), float(t.abs().mean()), float(t.std())])
    return np.array(st, np.float64)


def gen_e2e(out_dir, B=2, H=128, W=192):
    P = O.synthetic_params(0)
    batch = O.synthetic_batch(B, H, W, 1234)
    d = {"weight_checksum": np.array([float(sum(v.double().sum() for v in P.values())),
                                      float(sum(v.double().abs().sum() for v in P.values()))]),
         "input_checksum": np.array([float(batch[k].double().sum()) for k in
                                     ("input1", "input2", "target1", "target2", "target_occ1", "target_occ2")])}
    names = sorted(P.keys())
    d["param_names"] = np.array(names)
    for mode, robust in (("asis", False), ("robust", True)):
        # eval, as-is reference (unpatched rescale)
        set_mode(False, robust)
        m, args = ref_model(P)
        m.eval()
        with torch.no_grad():
            ev = m({"input1": batch["input1"], "input2": batch["input2"]})
        d[f"{mode}_eval_flow"] = npf(ev["flow"])
        d[f"{mode}_eval_occ"] = npf(ev["occ"])
        lossm = losses.MultiScaleEPE_PWC_Bi_Occ_upsample(args)
        lossm.eval()
        em = lossm(ev, batch)
        d[f"{mode}_eval_metrics"] = np.array([float(em["epe"]), float(em["F1"])])
        # eval with the alias patch must be bit-identical (finding 3)
        set_mode(True, robust)
        with torch.no_grad():
            ev2 = m({"input1": batch["input1"], "input2": batch["input2"]})
        assert torch.equal(ev["flow"], ev2["flow"]) and torch.equal(ev["occ"], ev2["occ"]), "alias patch changed eval"
        # train step quantities
        m.train()
        lossm.train()
        out = m({"input1": batch["input1"].clone().requires_grad_(True),
                 "input2": batch["input2"].clone().requires_grad_(True)})
        ld = lossm(out, batch)
        ld["total_loss"].backward()
        sd = dict(m.named_parameters())
        d[f"{mode}_train_losses"] = np.array([float(ld["flow_loss"]), float(ld["occ_loss"]), float(ld["total_loss"])])
        d[f"{mode}_train_gradnorm"] = np.array([float(sd[n].grad.double().norm()) for n in names])
        d[f"{mode}_train_gradsum"] = np.array([float(sd[n].grad.double().sum()) for n in names])
        d[f"{mode}_train_outstats"] = _flat_stats(out)
        # level-4 outputs in full for one sample (flow_f refined + occ_f refined), and finest occ
        d[f"{mode}_train_l4_flow_f"] = npf(out["flow"][4][2][:1])
        d[f"{mode}_train_l4_occ_f"] = npf(out["occ"][4][2][:1])
        d[f"{mode}_train_l6_occ_f"] = npf(out["occ"][6][0][:1, :, ::4, ::4])
        # one Adam step, post-step parameter checksum (A14)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=4e-4)
        opt.step()
        d[f"{mode}_poststep_sum"] = np.array([float(sd[n].detach().double().sum()) for n in names])
        # Sintel-variant loss for the same outputs (secondary)
        m.zero_grad()
        out = m({"input1": batch["input1"], "input2": batch["input2"]})
        ls = losses.MultiScaleEPE_PWC_Bi_Occ_upsample_Sintel(args)
        ls.train()
        l2 = ls(out, batch)
        d[f"{mode}_train_losses_sintel"] = np.array([float(l2["flow_loss"]), float(l2["occ_loss"]), float(l2["total_loss"])])
    set_mode(False, False)
    np.savez_compressed(os.path.join(out_dir, f"e2e_B{B}_{H}x{W}.npz"), **d)
    # the two weight checksums summed exactly (math.fsum): independent of the reduction order of the host's torch build
    np.savez_compressed(os.path.join(out_dir, "weight_checksum_seed0.npz"),
                        weight_checksum_exact=np.array([math.fsum(v for t in P.values() for v in t.double().flatten().tolist()),
                                                        math.fsum(v for t in P.values() for v in t.double().abs().flatten().tolist())]))


def gen_e2e_big(out_dir, B=1, H=384, W=448):
    """384x448: 4096 sampled output pixels + stats, both modes, eval only."""
    P = O.synthetic_params(0)
    batch = O.synthetic_batch(B, H, W, 1234)
    g = torch.Generator().manual_seed(99)
    idx = torch.randperm(H * W, generator=g)[:4096]
    d = {"sample_idx": idx.numpy()}
    for mode, robust in (("asis", False), ("robust", True)):
        set_mode(False, robust)
        m, _ = ref_model(P)
        m.eval()
        with torch.no_grad():
            ev = m({"input1": batch["input1"], "input2": batch["input2"]})
        d[f"{mode}_flow_samples"] = npf(ev["flow"].reshape(B, 2, -1)[:, :, idx])
        d[f"{mode}_occ_samples"] = npf(ev["occ"].reshape(B, 1, -1)[:, :, idx])
        d[f"{mode}_stats"] = np.array([float(ev["flow"].mean()), float(ev["flow"].abs().mean()),
                                       float(ev["occ"].mean()), float(ev["occ"].abs().mean())])
    set_mode(False, False)
    np.savez_compressed(os.path.join(out_dir, f"e2e_B{B}_{H}x{W}.npz"), **d)


def gen_e2e_train_x3(out_dir, B=4, H=384, W=448):
    """Train step at a size where the build's DEFAULT routing sends the level-4 decoder / context / refine layers to the
    bf16x3-split kernels (2B = 8 samples of 96x112: 384 blocks, 86 016 pixels) -- robust-mask mode: losses, 124 gradient
    norms / sums, post-Adam parameter checksums, and the level-4 / full-resolution outputs of sample 0."""
    P = O.synthetic_params(0)
    batch = O.synthetic_batch(B, H, W, 1234)
    names = sorted(P.keys())
    d = {"param_names": np.array(names)}
    set_mode(True, True)
    m, args = ref_model(P)
    args.batch_size = B
    m.train()
    lossm = losses.MultiScaleEPE_PWC_Bi_Occ_upsample(args)
    lossm.train()
    out = m({"input1": batch["input1"].clone().requires_grad_(True), "input2": batch["input2"].clone().requires_grad_(True)})
    ld = lossm(out, batch)
    ld["total_loss"].backward()
    sd = dict(m.named_parameters())
    d["robust_train_losses"] = np.array([float(ld["flow_loss"]), float(ld["occ_loss"]), float(ld["total_loss"])])
    d["robust_train_gradnorm"] = np.array([float(sd[n].grad.double().norm()) for n in names])
    d["robust_train_gradsum"] = np.array([float(sd[n].grad.double().sum()) for n in names])
    d["robust_train_l4_flow_f"] = npf(out["flow"][4][2][:1])
    d["robust_train_l4_occ_f"] = npf(out["occ"][4][2][:1])
    d["robust_train_l6_flow_f"] = npf(out["flow"][6][0][:1, :, ::4, ::4])
    d["robust_train_l6_occ_f"] = npf(out["occ"][6][0][:1, :, ::4, ::4])
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=4e-4)
    opt.step()
    d["robust_poststep_sum"] = np.array([float(sd[n].detach().double().sum()) for n in names])
    set_mode(False, False)
    print("train losses", d["robust_train_losses"], "grad-L2", float(np.sqrt((d["robust_train_gradnorm"] ** 2).sum())))
    np.savez_compressed(os.path.join(out_dir, f"e2e_train_B{B}_{H}x{W}.npz"), **d)


TRAIN3_SEEDS = (1234, 99, 7)
TRAIN3_FULL = ("conv_1x1_1.0.bias", "conv_1x1_1.0.weight", "flow_estimators.conv_last.0.bias", "flow_estimators.conv_last.0.weight",
               "occ_shuffle_upsample.out_convs.0.weight", "feature_pyramid_extractor.convs.0.0.0.bias",
               "refine_flow.convs.6.0.bias", "context_networks.convs.6.0.weight")


def gen_train3(out_dir, B=2, H=128, W=192):
    """THREE consecutive optimisation steps of the reference (runtime.py:158-189 with torch.optim.Adam(lr 1e-4, weight_decay 4e-4),
    scripts/IRR-PWC_flyingChairsOcc.sh:29-31) on three DIFFERENT batches (seeds 1234 / 99 / 7), robust-mask mode.  After the
    first step Adam is lr*sign(g) whatever its hyper-parameters are; steps 2-3 on fresh batches make beta1, beta2, both bias
    corrections and the weight-decay term observable.  Stored: the three loss triples, for every parameter the L2 norm of
    (parameter after step 3 - initial parameter) and of (after step 3 - after step 1), and a few small tensors in full."""
    P = O.synthetic_params(0)
    names = sorted(P.keys())
    set_mode(True, True)
    m, args = ref_model(P)
    args.batch_size = B
    m.train()
    lossm = losses.MultiScaleEPE_PWC_Bi_Occ_upsample(args)
    lossm.train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=4e-4)
    sd = dict(m.named_parameters())
    init = {n: sd[n].detach().double().clone() for n in names}
    d = {"param_names": np.array(names), "seeds": np.array(TRAIN3_SEEDS), "full_names": np.array(TRAIN3_FULL)}
    ls = []
    after1 = None
    for it, seed in enumerate(TRAIN3_SEEDS):
        batch = O.synthetic_batch(B, H, W, seed)
        for k, t in batch.items():                              # runtime.py:158-162
            t.requires_grad_("input" in k)
        opt.zero_grad()
        ld = lossm(m(batch), batch)
        ld["total_loss"].backward()
        opt.step()
        ls.append([float(ld["flow_loss"]), float(ld["occ_loss"]), float(ld["total_loss"])])
        if it == 0:
            after1 = {n: sd[n].detach().double().clone() for n in names}
    d["losses"] = np.array(ls)
    d["delta_norm_3_vs_init"] = np.array([float((sd[n].detach().double() - init[n]).norm()) for n in names])
    d["delta_norm_3_vs_1"] = np.array([float((sd[n].detach().double() - after1[n]).norm()) for n in names])
    d["delta_sum_3_vs_init"] = np.array([float((sd[n].detach().double() - init[n]).sum()) for n in names])
    for n in TRAIN3_FULL:
        d["full_" + n] = (sd[n].detach().double() - init[n]).numpy()          # the DELTA, float64
    set_mode(False, False)
    print("train3 losses", d["losses"].tolist(), "total delta", float(np.sqrt((d["delta_norm_3_vs_init"] ** 2).sum())))
    np.savez_compressed(os.path.join(out_dir, f"train3_B{B}_{H}x{W}.npz"), **d)


def gen_train_448x1024(out_dir, B=1, H=448, W=1024):
    """One train step at the second crop of north_star (Sintel-shaped 448x1024, BASELINE configs[4]), B = 1, robust-mask mode:
    losses, the 124 gradient norms / sums and subsampled level-4 / full-resolution outputs."""
    P = O.synthetic_params(0)
    batch = O.synthetic_batch(B, H, W, 1234)
    names = sorted(P.keys())
    d = {"param_names": np.array(names)}
    set_mode(True, True)
    m, args = ref_model(P)
    args.batch_size = B
    m.train()
    lossm = losses.MultiScaleEPE_PWC_Bi_Occ_upsample(args)
    lossm.train()
    out = m({"input1": batch["input1"].clone().requires_grad_(True), "input2": batch["input2"].clone().requires_grad_(True)})
    ld = lossm(out, batch)
    ld["total_loss"].backward()
    sd = dict(m.named_parameters())
    d["robust_train_losses"] = np.array([float(ld["flow_loss"]), float(ld["occ_loss"]), float(ld["total_loss"])])
    d["robust_train_gradnorm"] = np.array([float(sd[n].grad.double().norm()) for n in names])
    d["robust_train_gradsum"] = np.array([float(sd[n].grad.double().sum()) for n in names])
    d["robust_train_l4_flow_f"] = npf(out["flow"][4][2][:1, :, ::2, ::2])
    d["robust_train_l4_occ_b"] = npf(out["occ"][4][3][:1, :, ::2, ::2])
    d["robust_train_l6_flow_b"] = npf(out["flow"][6][1][:1, :, ::8, ::8])
    d["robust_train_l6_occ_f"] = npf(out["occ"][6][0][:1, :, ::8, ::8])
    set_mode(False, False)
    print("448x1024 train losses", d["robust_train_losses"], "grad-L2", float(np.sqrt((d["robust_train_gradnorm"] ** 2).sum())))
    np.savez_compressed(os.path.join(out_dir, f"e2e_train_B{B}_{H}x{W}.npz"), **d)


def gen_oddsize(out_dir):
    """Inputs whose height / width are NOT multiples of 64 (the reference evaluates Sintel 436x1024 and KITTI ~375x1242 as
    they come, scripts/validation/IRR-PWC_sintel.sh:17-29): odd pyramid sizes (436 -> 218, 109, 55, 28, 14, 7), the
    bilinear align_corners=False fallback of upsample_factor2 (models/irr_modules.py:21-27) and adaptive_avg_pool2d with
    non-integer ratios in the loss (losses.py:16-18).  Robust-mask mode.
    (i) 436x1024 and 375x1242, B = 1, eval: 4096 sampled output pixels + stats; (ii) 100x132, B = 2: eval outputs in full,
    one train step (losses, 124 gradient norms, post-Adam checksums)."""
    P = O.synthetic_params(0)
    d = {}
    set_mode(False, True)
    for H, W in ((436, 1024), (375, 1242)):
        batch = O.synthetic_batch(1, H, W, 1234)
        idx = torch.randperm(H * W, generator=torch.Generator().manual_seed(99))[:4096]
        m, _ = ref_model(P)
        m.eval()
        with torch.no_grad():
            ev = m({"input1": batch["input1"], "input2": batch["input2"]})
        k = f"{H}x{W}"
        d[k + "_idx"] = idx.numpy()
        d[k + "_flow_samples"] = npf(ev["flow"].reshape(1, 2, -1)[:, :, idx])
        d[k + "_occ_samples"] = npf(ev["occ"].reshape(1, 1, -1)[:, :, idx])
        d[k + "_stats"] = np.array([float(ev["flow"].mean()), float(ev["flow"].abs().mean()), float(ev["occ"].mean())])
        print(k, d[k + "_stats"], flush=True)
    B, H, W = 2, 100, 132
    batch = O.synthetic_batch(B, H, W, 1234)
    names = sorted(P.keys())
    d["param_names"] = np.array(names)
    m, args = ref_model(P)
    m.eval()
    with torch.no_grad():
        ev = m({"input1": batch["input1"], "input2": batch["input2"]})
    d["small_eval_flow"], d["small_eval_occ"] = npf(ev["flow"]), npf(ev["occ"])
    set_mode(True, True)
    m.train()
    lossm = losses.MultiScaleEPE_PWC_Bi_Occ_upsample(args)
    lossm.train()
    out = m({"input1": batch["input1"].clone().requires_grad_(True), "input2": batch["input2"].clone().requires_grad_(True)})
    d["small_train_sizes"] = np.array([list(lv[0].shape[2:]) for lv in out["flow"]])
    ld = lossm(out, batch)
    ld["total_loss"].backward()
    sd = dict(m.named_parameters())
    d["small_train_losses"] = np.array([float(ld["flow_loss"].detach()), float(ld["occ_loss"].detach()), float(ld["total_loss"].detach())])
    d["small_train_gradnorm"] = np.array([float(sd[n].grad.double().norm()) for n in names])
    opt = torch.optim.Adam(m.parameters(), lr=1e-4, weight_decay=4e-4)
    opt.step()
    d["small_poststep_sum"] = np.array([float(sd[n].detach().double().sum()) for n in names])
    set_mode(False, False)
    print("small", d["small_train_sizes"].tolist(), d["small_train_losses"])
    np.savez_compressed(os.path.join(out_dir, "oddsize.npz"), **d)


def gen_init(out_dir):
    """Fingerprint of the reference's own MSRA init under torch.manual_seed(0)."""
    m, _ = ref_model(None, seed=0)
    sd = m.state_dict()
    names = list(sd.keys())
    np.savez_compressed(os.path.join(out_dir, "init_seed0.npz"), names=np.array(names),
                        shapes=np.array([str(tuple(sd[n].shape)) for n in names]),
                        sums=np.array([float(sd[n].double().sum()) for n in names]),
                        abssums=np.array([float(sd[n].double().abs().sum()) for n in names]),
                        # the same fingerprints summed exactly (math.fsum): independent of the reduction order of the host's torch build
                        fsums=np.array([math.fsum(sd[n].double().flatten().tolist()) for n in names]),
                        fabssums=np.array([math.fsum(sd[n].double().abs().flatten().tolist()) for n in names]),
                        n_params=np.array([sum(v.numel() for v in sd.values())]))


def gen_pwcnet_plumbing(out_dir):
    """BASELINE config 0: pwcnet.py forward on one random 128x192 pair (plumbing), as-is and robust-mask modes,
    plus the reference's own as-is noise (8 vs 1 CPU threads)."""
    args = types.SimpleNamespace(batch_size=1, model_div_flow=0.05)
    g = torch.Generator().manual_seed(4321)
    i1 = torch.rand(1, 3, 128, 192, generator=g)
    i2 = torch.rand(1, 3, 128, 192, generator=g)
    d = {}
    for mode, robust in (("asis", False), ("robust", True)):
        set_mode(False, robust)
        torch.manual_seed(0)
        m = models.PWCNet(args)
        m.eval()
        outs = []
        for th in (8, 1):
            torch.set_num_threads(th)
            with torch.no_grad():
                outs.append(m({"input1": i1, "input2": i2})["flow"])
        torch.set_num_threads(8)
        d[f"{mode}_flow"] = npf(outs[0])
        d[f"{mode}_self_epe"] = np.array([float(torch.norm(outs[0] - outs[1], dim=1).mean())])
    set_mode(False, False)
    d["flow"] = d["asis_flow"]
    d["stats"] = np.array([float(np.mean(d["asis_flow"])), float(np.abs(d["asis_flow"]).mean())])
    print({k: float(v[0]) for k, v in d.items() if k.endswith("self_epe")}, d["stats"])
    np.savez_compressed(os.path.join(out_dir, "pwcnet_plumbing.npz"), **d)


def gen_noise_floor(out_dir, B=2, H=128, W=192):
    """Reference self-noise in as-is mode (mask >= 1.0): the SAME reference model evaluated with 8 and with 1
    CPU threads (different summation orders inside MKL-DNN) -- the yardstick for as-is parity (SURVEY finding 4)."""
    P = O.synthetic_params(0)
    batch = O.synthetic_batch(B, H, W, 1234)
    res = {}
    for mode, robust in (("asis", False), ("robust", True)):
        set_mode(False, robust)
        m, _ = ref_model(P)
        m.eval()
        outs = []
        for th in (8, 1):
            torch.set_num_threads(th)
            with torch.no_grad():
                outs.append(m({"input1": batch["input1"], "input2": batch["input2"]})["flow"])
        torch.set_num_threads(8)
        res[f"{mode}_self_epe_8thr_vs_1thr"] = np.array([float(torch.norm(outs[0] - outs[1], dim=1).mean())])
    # round 5: the same yardstick for the TRAIN step in as-is mode (VERDICT r4 missing #3): losses and the 124 gradient norms of the
    # reference's own step (alias-preserving rescale patch, mask >= 1.0) with 8 and with 1 CPU threads -- the mask discontinuity makes
    # the reference differ from itself; a build is at parity when it is no further from the 8-thread run than twice that
    names = sorted(P.keys())
    for th in (8, 1):
        torch.set_num_threads(th)
        set_mode(True, False)
        m, args = ref_model(P)
        m.train()
        lossm = losses.MultiScaleEPE_PWC_Bi_Occ_upsample(args)
        lossm.train()
        out = m({"input1": batch["input1"].clone().requires_grad_(True), "input2": batch["input2"].clone().requires_grad_(True)})
        ld = lossm(out, batch)
        ld["total_loss"].backward()
        sd = dict(m.named_parameters())
        res[f"asis_train_losses_{th}thr"] = np.array([float(ld["flow_loss"]), float(ld["occ_loss"]), float(ld["total_loss"])])
        res[f"asis_train_gradnorm_{th}thr"] = np.array([float(sd[n].grad.double().norm()) for n in names])
    torch.set_num_threads(8)
    res["param_names"] = np.array(names)
    set_mode(False, False)
    np.savez_compressed(os.path.join(out_dir, "noise_floor.npz"), **res)
    print({k: float(v[0]) for k, v in res.items() if k.endswith("1thr") and v.size == 1},
          res["asis_train_losses_8thr"], res["asis_train_losses_1thr"])


def _corr_scalar(f1, f2, pad, k, md, s1, s2):
    """loop-for-loop transcription of the forward kernel (models/correlation_package/correlation_cuda_kernel.cu:41-114, channels-last
    padded copies as in :15-39, output shape correlation_cuda.cc:23-32) in plain Python: the golden values for the parameter points the
    reference's Python path does not cover"""
    import math
    B, C, H, W = f1.shape
    kr, dr = (k - 1) // 2, md // s2
    D = 2 * dr + 1
    pH, pW = H + 2 * pad, W + 2 * pad
    OH = math.ceil((pH - 2 * (kr + md)) / s1)
    OW = math.ceil((pW - 2 * (kr + md)) / s1)
    P1 = torch.zeros(B, pH, pW, C, dtype=f1.dtype)
    P2 = torch.zeros_like(P1)
    P1[:, pad:pad + H, pad:pad + W] = f1.permute(0, 2, 3, 1)
    P2[:, pad:pad + H, pad:pad + W] = f2.permute(0, 2, 3, 1)
    zero = torch.zeros(C, dtype=f1.dtype)
    at = lambda P, n, y, x: P[n, y, x] if (0 <= y < pH and 0 <= x < pW) else zero
    out = torch.zeros(B, D * D, OH, OW, dtype=f1.dtype)
    for n in range(B):
        for oy in range(OH):
            for ox in range(OW):
                y1, x1 = oy * s1 + md, ox * s1 + md
                for tj in range(-dr, dr + 1):
                    for ti in range(-dr, dr + 1):
                        acc = 0.0
                        for j in range(-kr, kr + 1):
                            for i in range(-kr, kr + 1):
                                acc += float((at(P1, n, y1 + j, x1 + i) * at(P2, n, y1 + tj * s2 + j, x1 + ti * s2 + i)).sum())
                        out[n, (tj + dr) * D + (ti + dr), oy, ox] = acc / (k * k * C)
    return out


CORR_GENERAL_POINTS = [(3, 3, 4, 1, 2), (2, 1, 2, 2, 1), (4, 3, 2, 2, 2), (0, 1, 0, 1, 1), (1, 3, 1, 1, 1), (20, 1, 20, 1, 2)]


def gen_corr_general(out_dir):
    """The legacy Correlation operator off the IRR-PWC point (VERDICT r4 missing #4).  (a) points (md, 1, md, 1, 1): the imported
    reference's Python path compute_cost_volume (models/pwc_modules.py:42-62) incl. its autograd gradients; (b) the other points: the
    scalar transcription above (the CUDA operator itself cannot be built or run here).  fp64 inputs are stored (tiny)."""
    g = torch.Generator().manual_seed(77)
    f1 = torch.randn(2, 5, 9, 11, generator=g, dtype=torch.float64)
    f2 = torch.randn(2, 5, 9, 11, generator=g, dtype=torch.float64)
    d = {"f1": f1.numpy(), "f2": f2.numpy()}
    for md in (1, 2, 3):
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        o = ref_pwc.compute_cost_volume(a, b, {"max_disp": md})
        go = torch.randn(o.shape, generator=g, dtype=torch.float64)
        o.backward(go)
        d.update({f"ref_md{md}_out": o.detach().numpy(), f"ref_md{md}_go": go.numpy(), f"ref_md{md}_g1": a.grad.numpy(),
                  f"ref_md{md}_g2": b.grad.numpy()})
    for pt in CORR_GENERAL_POINTS:
        d["scalar_" + "_".join(map(str, pt))] = _corr_scalar(f1, f2, *pt).numpy()
    np.savez_compressed(os.path.join(out_dir, "corr_general.npz"), **d)
    print({k: v.shape for k, v in d.items()})


def gen_augment(out_dir):
    """RandomAffineFlowOcc of the imported reference (CPU; seeds fixed) -> inputs, sampled thetas and outputs.
    Cases: no noise / no crop; no noise + crop; noise (only the thetas and the noise-free tensors are comparable)."""
    import augmentations as ref_aug
    import augment_oracle  # noqa: F401  (import check only)
    d = {}
    for name, (B, H, W, noise, crop, seed) in {"plain": (3, 48, 64, False, None, 11), "crop": (2, 64, 96, False, [48, 64], 12),
                                               "noise": (2, 32, 48, True, None, 13)}.items():
        g = torch.Generator().manual_seed(100 + seed)
        ex = {"input1": torch.rand(B, 3, H, W, generator=g), "input2": torch.rand(B, 3, H, W, generator=g),
              "target1": 4 * torch.randn(B, 2, H, W, generator=g), "target2": 4 * torch.randn(B, 2, H, W, generator=g),
              "target_occ1": (torch.rand(B, 1, H, W, generator=g) < 0.3).float(),
              "target_occ2": (torch.rand(B, 1, H, W, generator=g) < 0.3).float()}
        for k, v in ex.items():
            d[f"{name}_in_{k}"] = npf(v)
        aug = ref_aug.RandomAffineFlowOcc(types.SimpleNamespace(), addnoise=noise, crop=crop)
        captured = []
        orig = aug.apply_random_transforms_to_params

        def wrapped(*a, **k):
            t = orig(*a, **k)
            captured.append(t.clone())
            return t
        aug.apply_random_transforms_to_params = wrapped
        torch.manual_seed(seed)
        np.random.seed(seed)
        out = aug({k: v.clone() for k, v in ex.items()})
        d[f"{name}_theta1_sampled"] = npf(captured[0])
        d[f"{name}_theta2_sampled"] = npf(captured[1])
        for k in ex:
            d[f"{name}_out_{k}"] = npf(out[k])
        d[f"{name}_cfg"] = np.array([B, H, W, int(noise), crop[0] if crop else 0, crop[1] if crop else 0, seed], np.int64)
    np.savez_compressed(os.path.join(out_dir, "augment.npz"), **d)


VARIANTS = [("PWCNet_bi", "MultiScaleEPE_PWC_Bi"), ("PWCNet_occ", "MultiScaleEPE_PWC_Occ"), ("PWCNet_occ_bi", "MultiScaleEPE_PWC_Bi_Occ"),
            ("PWCNet_irr", "MultiScaleEPE_PWC"), ("PWCNet_irr_bi", "MultiScaleEPE_PWC_Bi"), ("PWCNet_irr_occ", "MultiScaleEPE_PWC_Occ"),
            ("PWCNet_irr_occ_bi", "MultiScaleEPE_PWC_Bi_Occ")]


def _rescale_pure(flow, div_flow, width_im, height_im, to_local=True):
    """autograd-legal twin of rescale_flow for the ablation models, where every call site rebinds the name."""
    if to_local:
        u, v = float(flow.size(3) / width_im / div_flow), float(flow.size(2) / height_im / div_flow)
    else:
        u, v = float(width_im * div_flow / flow.size(3)), float(height_im * div_flow / flow.size(2))
    return flow * torch.tensor([u, v]).view(1, 2, 1, 1)


def variant_batch(B=1, H=128, W=192, seed=4321):
    g = torch.Generator().manual_seed(seed)
    return {"input1": torch.rand(B, 3, H, W, generator=g), "input2": torch.rand(B, 3, H, W, generator=g),
            "target1": 5 * torch.randn(B, 2, H, W, generator=g), "target2": 5 * torch.randn(B, 2, H, W, generator=g),
            "target_occ1": (torch.rand(B, 1, H, W, generator=g) < 0.2).float(),
            "target_occ2": (torch.rand(B, 1, H, W, generator=g) < 0.2).float(),
            "input_valid": (torch.rand(B, 1, H, W, generator=g) < 0.6).float()}


def gen_variants(out_dir):
    """the seven pwcnet_* ablation models (reference MSRA init under seed 0, robust-mask mode):
    eval outputs (every second pixel), training losses with the matching loss class and the global gradient norm;
    plus the Sintel / KITTI fine-tuning losses on IRR_PWC training outputs."""
    args = types.SimpleNamespace(batch_size=1, model_div_flow=0.05)
    batch = variant_batch()
    d = {}
    set_mode(False, True)
    for mname, lname in VARIANTS:
        modname = "models." + mname.replace("PWCNet", "pwcnet")
        mod = sys.modules[modname]
        orig = getattr(mod, "rescale_flow", None)
        if orig is not None:
            mod.rescale_flow = _rescale_pure
        torch.manual_seed(0)
        m = getattr(models, mname)(args)
        sd = m.state_dict()
        d[f"{mname}_keys"] = np.array(list(sd.keys()))
        d[f"{mname}_init"] = np.array([float(sum(v.double().sum() for v in sd.values())), float(sum(v.double().abs().sum() for v in sd.values()))])
        m.eval()
        with torch.no_grad():
            out = m(batch)
        d[f"{mname}_flow"] = npf(out["flow"][:, :, ::2, ::2])
        d[f"{mname}_flow_stats"] = np.array([float(out["flow"].mean()), float(out["flow"].abs().mean())])
        if "occ" in out:
            d[f"{mname}_occ"] = npf(out["occ"][:, :, ::2, ::2])
        m.train()
        loss = getattr(losses, lname)(args).train()
        ld = loss(m(batch), batch)
        ld["total_loss"].backward()
        gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None)))
        d[f"{mname}_losses"] = np.array([float(ld.get("flow_loss", ld["total_loss"])), float(ld.get("occ_loss", 0.0)), float(ld["total_loss"]), gn])
        print(mname, d[f"{mname}_flow_stats"], d[f"{mname}_losses"], flush=True)
        if orig is not None:
            mod.rescale_flow = orig
    # fine-tuning losses on IRR_PWC training outputs
    set_mode(True, True)
    torch.manual_seed(0)
    m = models.IRR_PWC(args).train()
    for lname in ("MultiScaleEPE_PWC_Bi_Occ_upsample_Sintel", "MultiScaleEPE_PWC_Bi_Occ_upsample_KITTI"):
        m.zero_grad()
        ld = getattr(losses, lname)(args).train()(m(batch), batch)
        ld["total_loss"].backward()
        gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in m.parameters() if p.grad is not None)))
        d[f"{lname}_losses"] = np.array([float(ld["flow_loss"]), float(ld.get("occ_loss", 0.0)), float(ld["total_loss"]), gn])
        print(lname, d[f"{lname}_losses"], flush=True)
    # KITTI eval metrics on a synthetic prediction
    g = torch.Generator().manual_seed(9)
    pred = {"flow": batch["target1"] + 3 * torch.randn(1, 2, 128, 192, generator=g), "occ": torch.randn(1, 1, 128, 192, generator=g)}
    le = losses.MultiScaleEPE_PWC_Bi_Occ_upsample_KITTI(args).eval()(pred, batch)
    d["kitti_eval"] = np.array([float(le["epe"]), float(le["outlier"])])
    d["kitti_eval_pred_flow"] = npf(pred["flow"])
    set_mode(False, False)
    np.savez_compressed(os.path.join(out_dir, "variants.npz"), **d)


def gen_flowvis(out_dir):
    """Middlebury colour coding of utils/flow.py (pure numpy).  The module also imports pypng, which
    is absent here and only used by its PNG writer: an EMPTY placeholder module satisfies that import; no function of
    it is called."""
    if "png" not in sys.modules:
        sys.modules["png"] = types.ModuleType("png")
    import utils.flow as uf
    g = torch.Generator().manual_seed(21)
    flow = (6 * torch.randn(2, 24, 32, generator=g)).numpy().astype(np.float32)
    flow[:, 3, 4] = 0.0
    flow[0, 5, 6] = 2e7                                        # "unknown" marker
    d = {"flow": flow.copy(), "rgb": uf.flow_to_png_middlebury(flow.copy()), "wheel": uf.make_color_wheel()}
    np.savez_compressed(os.path.join(out_dir, "flowvis.npz"), **d)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "tests", "golden"))
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    torch.set_num_threads(8)
    steps = {"ops": gen_ops, "init": gen_init, "e2e": gen_e2e, "big": gen_e2e_big, "trainx3": gen_e2e_train_x3, "train3": gen_train3, "train448": gen_train_448x1024, "oddsize": gen_oddsize, "pwcnet": gen_pwcnet_plumbing, "noise": gen_noise_floor, "corrgen": gen_corr_general, "augment": gen_augment, "variants": gen_variants, "flowvis": gen_flowvis}
    for k, fn in steps.items():
        if a.only and k not in a.only.split(","):
            continue
        print("generating", k, flush=True)
        fn(a.out)
    print("done")

