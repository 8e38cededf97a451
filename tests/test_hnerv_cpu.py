"""CPU suite of the HNeRV baseline (reference model_hnerv.py:11-175, `--model HNeRV --optim_type Adam`): construction parity with the
reference, the plain-torch restatement (tests/hnerv_ref.py) against golden vectors of the REAL reference (tools/make_hnerv_goldens.py),
the additive C-ABI entry points, the fused Adam's state_dict layout, and the recipes' command lines."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import hnerv_ref
from conftest import ROOT, check_summary, group, load_golden

RT, AT = 1e-4, 1e-5      # CPU-vs-CPU, same ATen kernels (as tests/test_oracle_vs_golden.py)


@pytest.mark.parametrize("name,cfg", [("tiny", hnerv_ref.tiny_args), ("h1", hnerv_ref.h1_args)])
def test_hnerv_construction_matches_reference(name, cfg):
    from boosting_nerv_amd.model_hnerv import HNeRV, HNeRVDecoder
    npz = load_golden(f"hnerv_base_{name}.npz")
    torch.manual_seed(1)
    model = HNeRV(cfg())
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in npz["keys"]]
    assert hnerv_ref.decoder_sha(sd) == str(npz["decoder_sha256"])
    if name == "h1":
        assert abs(model.decoder_params() - float(npz["decoder_params"])) < 1e-9
        assert tuple(sd["decoder.5.conv.upconv.0.weight"].shape) == (156, 47, 5, 5)
    dec = HNeRVDecoder(model)
    assert dec.decoder is model.decoder and dec.head_layer is model.head_layer


def test_hnerv_refuses_the_forms_outside_the_path():
    from boosting_nerv_amd.model_hnerv import HNeRV
    for kw, word in ((dict(enc_strds=[]), "enc_strds"), (dict(conv_type=["pshuffel", "pshuffel"]), "conv_type"), (dict(quant=True), "quant")):
        a = hnerv_ref.tiny_args()
        a.__dict__.update(kw)
        with pytest.raises(NotImplementedError, match=word):
            HNeRV(a)


def test_restatement_reproduces_the_reference_tiny_model():
    npz = load_golden("hnerv_base_tiny.npz")
    sd = {k: v.clone().requires_grad_(True) for k, v in group(npz, "sd/").items()}
    frame = torch.rand(1, 3, 180, 320, generator=torch.Generator().manual_seed(int(npz["frame_seed"])))
    img, lst = hnerv_ref.forward(sd, frame, return_list=True)
    check_summary(img, npz, "img", RT, AT)
    for i, t in enumerate(lst):
        check_summary(t, npz, f"list{i}", RT, AT)
    loss = hnerv_ref.l2_loss(img, frame)
    assert abs(loss.item() - float(npz["loss_L2"])) < 1e-4 * abs(float(npz["loss_L2"]))
    from oracle import cpu_ref
    torch.testing.assert_close(cpu_ref.psnr_fn_single(img, frame), torch.from_numpy(npz["psnr"]), rtol=1e-5, atol=1e-4)
    loss.backward()
    for k, p in sd.items():
        if f"grad/{k}" not in npz.files:
            continue
        gn = float(npz[f"gnorm/{k}"])
        assert abs(p.grad.double().norm().item() - gn) <= 2e-3 * gn + 1e-7, k
        torch.testing.assert_close(p.grad, torch.from_numpy(npz[f"grad/{k}"]), rtol=2e-3, atol=1e-5 + 1e-4 * gn, msg=lambda m, k=k: f"{k}: {m}")


def test_restatement_reproduces_the_reference_adam_trajectory():
    from boosting_nerv_amd.synth import SyntheticVideo
    tiny = load_golden("hnerv_base_tiny.npz")
    npz = load_golden("hnerv_base_traj.npz")
    vid = SyntheticVideo(2, 180, 320)
    frames = torch.stack([vid.frame(i) for i in range(2)])
    losses, psnrs, final = hnerv_ref.trajectory(group(tiny, "sd/"), frames, npz["order"].tolist(), lr=float(npz["lr"]))
    for s, (l, p) in enumerate(zip(losses, psnrs)):
        assert abs(l - npz["loss"][s]) <= 1e-4 * abs(npz["loss"][s]), (s, l, npz["loss"][s])
        assert abs(p - npz["psnr"][s]) <= 1e-3, (s, p, npz["psnr"][s])
    for k, v in final.items():
        torch.testing.assert_close(v, torch.from_numpy(npz[f"final/{k}"]), rtol=1e-4, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


NEW_SYMBOLS = ("bnerv_conv5_igemm", "bnerv_conv5_ws_bytes", "bnerv_conv5_wgrad", "bnerv_conv5_wgrad_ws_bytes", "bnerv_gelu_fwd", "bnerv_mul",
               "bnerv_adam_table", "bnerv_adam_table_blocks")


def test_new_entry_points_are_declared_exported_and_bound():
    from boosting_nerv_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "bnerv.h")).read()
    lib = L.load()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in L.SYMBOLS and hasattr(lib, name), name
    assert lib.bnerv_abi_version() == 9


def _desc5(L, **kw):
    d = L.ConvDesc()
    one = C.c_void_p(16)                       # never dereferenced: validation fails before any launch
    d.x, d.w, d.out = one, one, one
    d.B, d.Cin, d.Cout, d.H, d.W, d.k = 1, 6, 24, 9, 16, 5
    d.in_mode, d.ep_mode, d.in_s, d.out_s, d.transposed, d.wCo, d.wCi = L.IN_PLAIN, L.EP_BIAS, 1, 2, 0, 24, 6
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    from boosting_nerv_amd import _lib as L
    lib = L.load()
    err = lambda: lib.bnerv_last_error().decode()
    ws = C.c_void_p(16)
    for kw, word in ((dict(k=3), "k must be 5"), (dict(out_s=3), "out_s must be 1 or 2"), (dict(x=None), "null"), (dict(ep_mode=L.EP_BIAS_SIN), "ep_mode"),
                     (dict(in_mode=L.IN_AFFINE), "in_mode"), (dict(wCi=7), "weight shape"), (dict(Cout=22, wCo=22), "divisible")):
        d = _desc5(L, **kw)
        assert lib.bnerv_conv5_igemm(None, C.byref(d), ws, 1 << 30) == -1 and word in err(), (kw, err())
    d = _desc5(L)
    assert lib.bnerv_conv5_igemm(None, C.byref(d), None, 0) == -1 and "workspace" in err()
    assert lib.bnerv_conv5_igemm(None, C.byref(d), ws, 16) == -3 and "workspace" in err()
    assert lib.bnerv_conv5_ws_bytes(6, 24) == 1 * 2 * 13 * 3 * 64 * 16 and lib.bnerv_conv5_ws_bytes(0, 4) == 0
    w = L.WgradDesc()
    w.x, w.g, w.dw, w.ws = ws, ws, ws, ws
    w.B, w.Cin, w.Cout, w.H, w.W, w.k, w.in_mode, w.g_mode, w.g_s = 1, 6, 24, 9, 16, 3, L.IN_PLAIN, L.IN_UNSHUFFLE, 2
    assert lib.bnerv_conv5_wgrad(None, C.byref(w)) == -1 and "k must be 5" in err()
    w.k, w.g_s = 5, 3
    assert lib.bnerv_conv5_wgrad(None, C.byref(w)) == -1 and "g_s must be 1 or 2" in err()
    w.g_s, w.ws_bytes = 2, 16
    assert lib.bnerv_conv5_wgrad(None, C.byref(w)) == -3 and "workspace" in err()
    assert lib.bnerv_conv5_wgrad_ws_bytes(1, 6, 24, 9, 16) == 2 * (25 * 24 * 6 + 24) * 4 and lib.bnerv_conv5_wgrad_ws_bytes(1, 6, 24, 0, 16) == 0
    assert lib.bnerv_adam_table(None, None, 1, 1, None) == -1 and "adam_table" in err()
    assert lib.bnerv_adam_table_blocks(5000) == lib.bnerv_adan_table_blocks(5000) == 5
    assert lib.bnerv_gelu_fwd(None, None, None, None, 4) == -1 and lib.bnerv_mul(None, None, None, None, 4) == -1
    # the 1x1 / 3x3 family is untouched: it still refuses k = 5
    d = _desc5(L)
    assert lib.bnerv_conv_igemm(None, C.byref(d)) == -1 and "k must be 1 or 3" in err()


def test_operator_and_module_refuse_what_the_kernels_do_not_cover():
    from boosting_nerv_amd import ops
    from boosting_nerv_amd.lib.quant_ops import CustomConv2d
    a = hnerv_ref.tiny_args()
    assert CustomConv2d(6, 24, 5, 1, 2, args=a).hip_supported() and not CustomConv2d(6, 24, 7, 1, 3, args=a).hip_supported()
    x, w = torch.zeros(1, 6, 4, 4), torch.zeros(54, 6, 5, 5)
    with pytest.raises(NotImplementedError, match="stride"):
        ops.upconv_act(x, w, None, 3, "gelu")
    with pytest.raises(NotImplementedError, match="act"):
        ops.upconv_act(x, torch.zeros(24, 6, 5, 5), None, 2, "relu")
    with pytest.raises(Exception, match="ROCm GPU"):           # no CPU fallback
        ops.upconv_act(x, torch.zeros(24, 6, 5, 5), None, 2, "gelu")


def test_fused_adam_state_dict_has_torch_adam_layout():
    from boosting_nerv_amd.optimizer import Adam
    ps = [torch.nn.Parameter(torch.randn(3, 4)), torch.nn.Parameter(torch.randn(5))]
    ours = Adam(ps, lr=1e-3)
    for i, p in enumerate(ps):                              # state as three steps would leave it (the launch itself needs the GPU)
        st = ours._ensure_state(p, 1, 1.0)
        st["exp_avg"].fill_(0.1 * (i + 1)); st["exp_avg_sq"].fill_(0.01 * (i + 1))
    ours.param_groups[0]["step"] = 3
    sd = ours.state_dict()
    assert set(sd["state"][0].keys()) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 3.0
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    stock = torch.optim.Adam(qs, lr=1e-3)
    stock.load_state_dict(sd)
    assert float(stock.state[qs[1]]["step"]) == 3.0 and torch.equal(stock.state[qs[1]]["exp_avg"], torch.full((5,), 0.2))
    for q in qs:
        q.grad = torch.ones_like(q)
    stock.step()                                            # a loaded stock optimizer really steps from that state
    back = Adam([torch.nn.Parameter(q.detach().clone()) for q in qs], lr=1e-3)
    back.load_state_dict(stock.state_dict())
    assert back.param_groups[0]["step"] == 4
    st = back.state[back.param_groups[0]["params"][0]]
    torch.testing.assert_close(st["exp_avg"], torch.full((3, 4), 0.9 * 0.1 + 0.1))
    assert back.param_groups[0]["betas"] == (0.9, 0.999) and back.param_groups[0]["eps"] == 1e-8
    with pytest.raises(NotImplementedError):
        Adam(ps, weight_decay=0.1)


RECIPE_COMMON = ("--model HNeRV --optim_type Adam --conv_type convnext pshuffel --act gelu --norm none --resize_list -1 --loss L2 "
                 "--enc_dim 64_16 --ks 0_1_5 --reduce 1.2 --dec_blks 1 1 1 1 1 -e 300 --eval_freq 30 --lower_width 12 -b 1 ")
RECIPES = {   # flag values of scripts/{regression/bunny,interpolation,inpanting}/hnerv.sh (settings only)
    "bunny": RECIPE_COMMON + "--outf regression/HNeRV/epoch_300 --data_path ./dataset/bunny --vid bunny --crop_list 720_1280 --enc_strds 5 2 2 2 2 "
                             "--dec_strds 5 2 2 2 2 --modelsize 1.525 --lr 0.001",
    "interpolation": RECIPE_COMMON + "--outf regression/HNeRV/epoch_300 --data_path ./dataset/UVG_Full/Beauty_1920x1080_120 --vid Beauty --crop_list 1080_1920 "
                                     "--enc_strds 5 3 2 2 2 --dec_strds 5 3 2 2 2 --modelsize 3.05 --lr 0.001 --interpolation --data_split 1_1_2 --embed_inter",
    "inpainting": RECIPE_COMMON + "--outf inpanting_center/HNeRV/epoch_300 --data_path ./dataset/DAVIS/JPEGImages/1080p/blackswan --vid blackswan "
                                  "--crop_list 1080_1920 --enc_strds 5 3 2 2 2 --dec_strds 5 3 2 2 2 --modelsize 3.0 --lr 0.0005 --inpanting inpanting_center "
                                  "--clip_max_norm 1",
}


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_cli_accepts_the_baseline_recipes(name):
    from boosting_nerv_amd import train_nerv_all as T
    a = T.build_parser().parse_args(RECIPES[name].split())
    assert a.model == "HNeRV" and a.optim_type == "Adam" and a.conv_type == ["convnext", "pshuffel"] and a.act == "gelu" and a.loss == "L2"
    assert a.ks == "0_1_5" and a.dec_blks == [1, 1, 1, 1, 1] and a.embed == "" and a.sft_block == "none" and a.norm == "none"
    if name == "interpolation":
        assert a.interpolation and a.embed_inter and a.data_split == "1_1_2"
    if name == "inpainting":
        assert a.inpanting == "inpanting_center" and a.clip_max_norm == 1


@pytest.mark.parametrize("crop,strds,frames,size,want", [("720_1280", [5, 2, 2, 2, 2], 132, 0.77, 59), ("720_1280", [5, 2, 2, 2, 2], 132, 1.525, 96),
                                                         ("720_1280", [5, 2, 2, 2, 2], 132, 3.05, 145), ("1080_1920", [5, 3, 2, 2, 2], 600, 3.05, 103)])
def test_size_solver_gives_the_baseline_widths(crop, strds, frames, size, want):
    from boosting_nerv_amd import train_nerv_all as T
    s = " ".join(str(x) for x in strds)
    a = T.build_parser().parse_args((RECIPE_COMMON + f"--crop_list {crop} --enc_strds {s} --dec_strds {s} --modelsize {size}").split())
    h, w = (int(x) for x in crop.split("_"))
    fc_dim, _ = T.solve_fc_dim(a, h * w, frames)
    assert fc_dim == want
