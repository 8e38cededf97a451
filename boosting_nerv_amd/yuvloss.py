"""The command-line side of the plane loss, shared by train_nerv_all.py and train_nerv_compression.py: the three flags, the
combinations no run can honour (refused with a ValueError before training starts), the record the steps take (engine.YuvTerm) and the log
texts.  The loss itself is csrc/yuv.hip behind ops.yuv420_loss / ops.yuv420_loss_value_grad_stats; yuvio.plane_loss_reference restates it.

    --yuv_loss LAMBDA         total loss = loss_fn(--loss) + LAMBDA * L          (default 0: off)
    --yuv_loss_weights 6_1_1  the plane weights of L
    --loss YUV420             L alone, times --yuv_loss (which then defaults to 1)
    --yuv_msssim LAMBDA       + LAMBDA * L_ms, the MS-SSIM-Y term of DESIGN section 37 (default 0: off; with or without --yuv_loss;
                              under --loss YUV420 the loss is yuv_loss * L + yuv_msssim * L_ms)
    --yuv_upscale             with --resize_list H_W: L is taken at the --crop_list size, the prediction up-sampled by the loader's own bicubic
                              inside the loss (ops.yuv420_up_loss); not with --yuv_msssim

Matrix, range and depth are the loader's (--yuv_matrix, --yuv_range, the file's format)."""
import numpy as np

PURE = "YUV420"


def add_flags(parser):
    parser.add_argument('--yuv_loss', type=float, default=0., metavar='LAMBDA',
                        help='add LAMBDA times the 4:2:0 plane loss against the raw .yuv source to the loss (0 = off; 1 under --loss YUV420)')
    parser.add_argument('--yuv_loss_weights', type=str, default='6_1_1', help='plane weights Y_U_V of the plane loss')
    parser.add_argument('--yuv_msssim', type=float, default=0., metavar='LAMBDA',
                        help='add LAMBDA times (1 - MS-SSIM of the luma plane against the raw .yuv source) to the loss (0 = off)')
    parser.add_argument('--yuv_upscale', action='store_true',
                        help='with --resize_list: take the plane loss at the --crop_list size, through the up-sampler (not with --yuv_msssim)')


def check_flags(args):
    """The parse-time half: normalises args.yuv_loss / args.yuv_loss_weights and refuses what needs no file to be refused."""
    from . import yuvio
    weights = yuvio.parse_weights(args.yuv_loss_weights)
    if not np.isfinite(args.yuv_loss) or args.yuv_loss < 0:
        raise ValueError(f"--yuv_loss {args.yuv_loss}: a factor >= 0 (0 switches the term off)")
    ms = float(getattr(args, "yuv_msssim", 0.0))
    if not np.isfinite(ms) or ms < 0:
        raise ValueError(f"--yuv_msssim {ms}: a factor >= 0 (0 switches the term off)")
    pure = args.loss == PURE
    if pure and args.yuv_loss == 0:
        args.yuv_loss = 1.0
    from .resize import parse_resize
    resize = parse_resize(getattr(args, "resize_list", "-1"))             # (ValueError for anything but -1 or H_W)
    if resize is not None and getattr(args, "embed_inter", False):
        raise ValueError(f"--resize_list {args.resize_list} with --embed_inter: the neighbour frames of a held-out frame come through the host loader "
                         "only; --embed_inter_stored interpolates from stored embeddings instead")
    up = bool(getattr(args, "yuv_upscale", False))
    if up and resize is None:
        raise ValueError("--yuv_upscale without --resize_list: the prediction already has the size of the source's window")
    if up and ms > 0:
        raise ValueError("--yuv_upscale with --yuv_msssim: the MS-SSIM-Y term has no form through the up-sampler")
    if up and not args.yuv_loss > 0:
        raise ValueError(f"--yuv_upscale without a plane loss: give --yuv_loss LAMBDA or --loss {PURE}")
    if not (args.yuv_loss > 0 or ms > 0):
        return args
    what = f"--loss {PURE}" if pure else ("--yuv_loss" if args.yuv_loss > 0 else "--yuv_msssim")
    if resize is not None and not up:
        raise ValueError(f"{what} with --resize_list {args.resize_list}: the raw source has no planes at the resized frame's size to compare against "
                         "(--yuv_upscale takes the plane loss at the --crop_list size, through the up-sampler)")
    if getattr(args, "inpanting", "none") != "none":
        raise ValueError(f"{what} with --inpanting {args.inpanting}: the plane loss has no masked form")
    if getattr(args, "host_frames", False) or getattr(args, "embed_inter", False):
        raise ValueError(f"{what} needs the clip resident on the device: drop --host_frames / --embed_inter")
    if not str(args.data_path).lower().endswith(".yuv"):
        raise ValueError(f"{what} compares against the planes of a raw source: --data_path {args.data_path} is no .yuv file")
    from .hnerv_utils import frame_hw
    h, w = tuple(int(x) for x in args.crop_list.split("_")[:2]) if up else frame_hw(args)      # (the window the planes are compared in)
    if h % 2 or w % 2:
        raise ValueError(f"{what}: 4:2:0 needs an even crop, --crop_list gives {h}x{w}")
    if ms > 0 and min(h, w) <= 160:
        raise ValueError(f"--yuv_msssim: the five-scale MS-SSIM needs min(H, W) > 160, --crop_list gives {h}x{w}")
    args.yuv_loss_weights = "_".join(f"{v:g}" for v in weights)
    return args


def make_term(args, dataset, device, resident):
    """engine.YuvTerm of this run, or None with the term off: uploads the raw clip beside the fp32 one.  Refuses (ValueError) a clip that is
    not resident or not raw, and a centre crop that starts at an odd row or column of the source."""
    from . import yuvio
    from .engine import YuvTerm
    ms = float(getattr(args, "yuv_msssim", 0.0))
    if not (getattr(args, "yuv_loss", 0) > 0 or ms > 0):
        return None
    what = f"--loss {PURE}" if args.loss == PURE else ("--yuv_loss" if getattr(args, "yuv_loss", 0) > 0 else "--yuv_msssim")
    if dataset.yuv is None:
        raise ValueError(f"{what} compares against the planes of a raw source: --data_path {args.data_path} is no .yuv file")
    if not resident:
        raise ValueError(f"{what} needs the clip resident on the device: drop --host_frames / --embed_inter")
    clip = dataset.yuv
    top, left, ch, cw = clip.crop_window((dataset.crop_h, dataset.crop_w))
    if top % 2 or left % 2 or ch % 2 or cw % 2:
        raise ValueError(f"{what}: the {cw}x{ch} centre crop of the {clip.width}x{clip.height} source starts at (top {top}, left {left}); offset and "
                         "size must be even, a chroma sample covers a 2x2 block of the source (choose --crop_list so that the margins are multiples of 4)")
    coeffs = yuvio.coefficients(dataset.yuv_matrix, dataset.yuv_range, clip.depth)
    raw = clip.raw_to_device(device, count=len(dataset.samples))
    if ms > 0 and min(ch, cw) <= 160:
        raise ValueError(f"--yuv_msssim: the five-scale MS-SSIM needs min(H, W) > 160, the crop is {ch}x{cw}")
    up = (ch, cw) if getattr(args, "yuv_upscale", False) else None
    return YuvTerm(raw, coeffs, (clip.height, clip.width), (top, left), weights=args.yuv_loss_weights, lam=args.yuv_loss, pure=args.loss == PURE, lam_ms=ms,
                   up=up)


def describe(term, frame_hw=None):
    """The run log's line; frame_hw: the size of the frames the run trains on (named with the term taken through the up-sampler)."""
    c = term.coeffs
    up = ""
    if getattr(term, "up", None) is not None:
        up = f", at {term.up[0]}x{term.up[1]} through the up-sampler" + ("" if frame_hw is None else f" (from {frame_hw[0]}x{frame_hw[1]})")
    return (f"YUV loss: lambda {term.lam:g}, weights {'_'.join(f'{v:g}' for v in term.weights)}, matrix {c.matrix}, range {c.range}, {c.depth} bit" + up
            + (f", MS-SSIM-Y lambda {term.lam_ms:g}" if term.lam_ms > 0 else "") + (" (pure: the RGB loss is off)" if term.pure else ""))


def psnr_text(stats):
    """'Y U V': -10 log10 of the batch-mean plane MSEs of a [B, 4] stats tensor (the PSNR of each plane before rounding to codes)."""
    mse = stats[:, 1:4].double().mean(dim=0).cpu().clamp_min(1e-20)
    return " ".join(f"{v:.2f}" for v in (-10.0 * mse.log10()).tolist())


def train_text(term, stats, ms=None):
    """What a train line carries behind its PSNR with the term on: ', yuv_psnr: Y U V' (with --yuv_loss) and ', yuv_msssim_y: v' (with
    --yuv_msssim; the batch mean of S)."""
    text = "" if stats is None else f", yuv_psnr: {psnr_text(stats)}"
    if term.lam_ms > 0 and ms is not None:
        text += f", yuv_msssim_y: {float(ms.double().mean().cpu()):.4f}"
    return text


def eager_term(term, out, img_idx):
    """(lam * L [+ lam_ms * L_ms] with its autograd node, stats) for the eager steps: sample b against raw frame img_idx[b].  With
    --yuv_msssim S [B] is left in term.ms_out, and stats is None where --yuv_loss is 0."""
    import torch
    sel = img_idx.reshape(-1).to(out.device, dtype=torch.float32)
    total, stats, _ = term.autograd_term(out, sel)
    return total, stats
