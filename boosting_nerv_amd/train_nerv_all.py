"""Train / eval driver -- drop-in for the reference's train_nerv_all.py: every flag of its CLI (train_nerv_all.py:28-110)
with the same defaults, the same derived fields (fc_dim solver :193-217, exp_id/outf :118-137), the same train loop
semantics (:322-410) and evaluate() metrics (:451-619), so scripts/regression/**.sh run unchanged.  Differences, all
MI355X-motivated and listed in DESIGN.md:
  * the step runs through engine.TrainStep (HIP kernels, hipGraph replay, device-side PSNR, no per-step host sync);
  * data parallelism is one flat-bucket RCCL all-reduce per step (dp.GradBucket) instead of DistributedDataParallel;
    launch with -d as the reference (mp.spawn) or under torchrun (RANK/WORLD_SIZE in the environment);
  * `--data_path synthetic:bunny|uvg|NxHxW` selects the in-repo synthetic clip; frames are kept resident in HBM;
  * evaluation metrics of all ranks are combined correctly (the reference drops the all-reduce result, :554-556).
TensorBoard, GIF dumps and the seaborn histogram branch are reporting-only and optional/absent."""
import argparse
import copy
import heapq
import os
import random
import shutil
import time

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.optim as optim
import torch.utils.data
from torch.utils.data import Subset

from . import ops
from . import runtime as rt
from . import yuvloss
from .dp import GradBucket
from .engine import TrainStep
from .hnerv_utils import TransformInput, VideoDataSet, adjust_lr, frame_hw, data_split, interp_plan, loss_fn, psnr_fn_device, quant_tensor, quant_tensor_sparse, worker_init_fn
from .model_enerv import ENeRV_Boost
from .model_hnerv import HNeRV, HNeRV_Boost
from .model_nerv import NeRV_Boost


def build_parser():
    parser = argparse.ArgumentParser()
    # Dataset parameters
    parser.add_argument('--data_path', type=str, default='', help='data path for vid (or synthetic:bunny|uvg|NxHxW)')
    parser.add_argument('--vid', type=str, default='k400_train0', help='video id')
    parser.add_argument('--shuffle_data', action='store_true', help='randomly shuffle the frame idx')
    parser.add_argument('--data_split', type=str, default='1_1_1', help='Valid_train/total_train/all data split')
    parser.add_argument('--crop_list', type=str, default='640_1280', help='video crop size')
    parser.add_argument('--resize_list', type=str, default='-1', help='video resize size')
    # architecture
    parser.add_argument('--model', type=str, default='', help='model name')
    parser.add_argument('--embed', type=str, default='', help='empty string for HNeRV, and base value/embed_length for NeRV position encoding')
    parser.add_argument('--ks', type=str, default='0_3_3', help='kernel size for encoder and decoder')
    parser.add_argument('--enc_blks', type=int, default=1, help='the number of encoder blocks')
    parser.add_argument('--enc_strds', type=int, nargs='+', default=[], help='stride list for encoder')
    parser.add_argument('--enc_dim', type=str, default='64_16', help='enc latent dim and embedding ratio')
    parser.add_argument('--modelsize', type=float, default=1.5, help='model parameters size: model size + embedding parameters')
    parser.add_argument('--saturate_stages', type=int, default=-1, help='saturate stages for model size computation')
    parser.add_argument('--lfreq', type=str, default="pi", help='frequency multiplier of the positional encoding')
    parser.add_argument('--fc_dim', type=int, default=None, help='channel width of the stem output')
    parser.add_argument('--fc_hw', type=str, default='9_16', help='out size (h,w) for mlp')
    parser.add_argument('--reduce', type=float, default=1.2, help='chanel reduction for next stage')
    parser.add_argument('--lower_width', type=int, default=32, help='lowest channel width for output feature maps')
    parser.add_argument('--dec_strds', type=int, nargs='+', default=[5, 3, 2, 2, 2], help='strides list for decoder')
    parser.add_argument('--dec_blks', type=int, nargs='+', default=[1, 1, 1, 1, 1], help='block number for decoder')
    parser.add_argument("--conv_type", default=['convnext', 'pshuffel'], type=str, nargs="+", help='conv type for encoder/decoder',
                        choices=['pshuffel', 'conv', 'convnext', 'interpolate', 'pshuffel_3x3'])
    parser.add_argument('--norm', default='none', type=str, help='norm layer for generator', choices=['none', 'bn', 'in'])
    parser.add_argument('--act', type=str, default='gelu', help='activation to use',
                        choices=['relu', 'leaky', 'leaky01', 'relu6', 'gelu', 'swish', 'softplus', 'hardswish', 'sin', 'ressin'])
    parser.add_argument('--sft_block', type=str, default='none', help='TAT block type')
    parser.add_argument('--ch_t', type=int, default=32, help='sft in channels')
    parser.add_argument('--block_dim', type=int, default=128, help='transformer dims in the enerv model')
    # training
    parser.add_argument('-j', '--workers', type=int, help='number of data loading workers', default=4)
    parser.add_argument('-b', '--batchSize', type=int, default=1, help='input batch size')
    parser.add_argument('--start_epoch', type=int, default=-1, help='starting epoch')
    parser.add_argument('--not_resume', action='store_true', help='not resume from latest checkpoint')
    parser.add_argument('-e', '--epochs', type=int, default=5, help='Epoch number')
    parser.add_argument('--block_params', type=str, default='1_1', help='residual blocks and percentile to save')
    parser.add_argument('--lr', type=float, default=0.001, help='learning rate')
    parser.add_argument('--lr_type', type=str, default='cosine_0.1_1_0.1', help='learning rate type')
    parser.add_argument('--loss', type=str, default='Fusion6', help='loss type')
    parser.add_argument('--out_bias', default='tanh', type=str, help='using sigmoid/tanh/0.5 for output prediction')
    parser.add_argument('--optim_type', default='adan', type=str, help='Adan | Adam')
    parser.add_argument('--clip_max_norm', default=0., type=float, help='clip_max_norm')
    parser.add_argument('--inpanting', default='none', type=str, help='do inpanting')
    parser.add_argument('--interpolation', action='store_true', default=False, help='do interpolation')
    parser.add_argument('--embed_inter', action='store_true', default=False, help='do interpolation')
    parser.add_argument('--embed_inter_stored', action='store_true', default=False,
                        help='with --interpolation (HNeRV, HNeRV_Boost), in place of --embed_inter: the embedding of every frame that is not a training '
                             'frame is derived from the embeddings of its nearest training frames in time, quantised as a file stores them, so '
                             '--bitstream writes the training frames\' embeddings only (DESIGN section 38)')
    parser.add_argument('--cabac', action='store_true', default=False)
    # global magnitude pruning with masked fine-tuning (prune.py); off by default
    parser.add_argument('--prune_sparsity', type=float, default=0., help='final total sparsity of the decoder weights, in [0, 1); 0 = no pruning')
    parser.add_argument('--prune_steps', type=int, nargs='+', default=[0],
                        help='epochs at whose start a prune event runs; event j of m prunes to 1 - (1 - S) ** ((j + 1) / m)')
    # evaluation
    parser.add_argument('--quant', action='store_true', default=False, help='enable quantization')
    parser.add_argument('--eval_only', action='store_true', default=False, help='do evaluation only')
    parser.add_argument('--eval_freq', type=int, default=10, help='evaluation frequency')
    parser.add_argument('--quant_model_bit', type=int, default=8, help='bit length for model quantization')
    parser.add_argument('--quant_embed_bit', type=int, default=6, help='bit length for embedding quantization')
    parser.add_argument('--quant_axis', type=int, default=0, help='quantization axis (-1 means per tensor)')
    parser.add_argument('--dump_images', action='store_true', default=False, help='dump the prediction images')
    parser.add_argument('--bitstream', type=str, default=None,
                        help='write the post-hoc quantised model of the final evaluation (and of --eval_only) to this file (codec.py decodes it)')
    parser.add_argument('--bitstream_sparse', action='store_true', default=False,
                        help='with --bitstream: quantise the prunable tensors so that a zero weight stays exactly zero and write the sparse file '
                             'kind, whose Huffman alphabet has leaves for runs of zeros (DESIGN section 31)')
    parser.add_argument('--bitstream_temporal', action='store_true', default=False,
                        help='with --bitstream (HNeRV, HNeRV_Boost): write the temporal file kind, in which a frame embedding is coded on its own or '
                             'as the differences to the frame before, each under a Huffman code of its own (DESIGN section 35); combines with '
                             '--bitstream_sparse')
    parser.add_argument('--dump_videos', action='store_true', default=False, help='concat the prediction images into video')
    parser.add_argument('--eval_fps', action='store_true', default=False, help='fwd multiple times to test the fps')
    parser.add_argument('--encoder_file', default='', type=str, help='specify the embedding file')
    parser.add_argument('--dump_values', action='store_true', default=False)
    parser.add_argument('--dump_features', action='store_true', default=False)
    # distributed
    parser.add_argument('--manualSeed', type=int, default=1, help='manual seed')
    parser.add_argument('-d', '--distributed', action='store_true', default=False, help='distributed training')
    # logging
    parser.add_argument('--debug', action='store_true', help='debug status, earlier for train/eval')
    parser.add_argument('-p', '--print-freq', default=50, type=int)
    parser.add_argument('--weight', default='None', type=str, help='pretrained weights for ininitialization')
    parser.add_argument('--overwrite', action='store_true', help='overwrite the output dir if already exists')
    parser.add_argument('--outf', default='unify', help='folder to output images and model checkpoints')
    parser.add_argument('--suffix', default='', help="suffix str for outf")
    # MI355X-side switches (not in the reference)
    parser.add_argument('--no_graph', action='store_true', help='disable hipGraph replay of the train step')
    parser.add_argument('--host_frames', action='store_true', help='stream frames through the DataLoader instead of keeping them in HBM')
    # a --data_path ending in .yuv is a raw planar YUV 4:2:0 clip (yuvio.py)
    parser.add_argument('--yuv_size', type=str, default=None, help='WxH of a raw .yuv clip (default: the _WxH_ of a UVG-style file name)')
    parser.add_argument('--yuv_fmt', type=str, default=None, choices=['yuv420p', 'yuv420p10le'], help='pixel format of a raw .yuv clip (default: 8bit / 10bit in its name)')
    parser.add_argument('--yuv_matrix', type=str, default='bt709', choices=['bt709', 'bt601'], help='colour matrix of a raw .yuv clip')
    parser.add_argument('--yuv_range', type=str, default='limited', choices=['limited', 'full'], help='sample range of a raw .yuv clip')
    # the plane loss against the raw source (yuvloss.py); off by default.  --loss YUV420 is its pure form
    yuvloss.add_flags(parser)
    return parser


def parse_args(argv=None):
    """The parsed command line, with the flag combinations no run can honour refused here (ValueError) instead of after the data is loaded."""
    args = build_parser().parse_args(argv)
    if not 0.0 <= args.prune_sparsity < 1.0:
        raise ValueError(f"--prune_sparsity {args.prune_sparsity}: a total sparsity in [0, 1)")
    steps = list(args.prune_steps)
    if not steps or len(set(steps)) != len(steps) or min(steps) < 0 or max(steps) >= max(args.epochs, 1):
        raise ValueError(f"--prune_steps {steps}: distinct epochs in [0, {args.epochs})")
    args.prune_steps = sorted(steps)
    if args.bitstream_sparse and not args.bitstream:
        raise ValueError("--bitstream_sparse: the sparse twin is what --bitstream FILE writes; give the file")
    if args.embed_inter_stored:
        if args.embed_inter:
            raise ValueError("--embed_inter_stored stands in place of --embed_inter (held-out embeddings from stored ones, not from the source frames): give one")
        if not args.interpolation:
            raise ValueError("--embed_inter_stored: the held-out frames it derives are those of an --interpolation run")
        if args.model not in ("HNeRV", "HNeRV_Boost"):
            raise ValueError(f"--embed_inter_stored: --model {args.model} has no frame embeddings to derive (HNeRV, HNeRV_Boost)")
        if args.shuffle_data:
            raise ValueError("--embed_inter_stored: --shuffle_data permutes the frames before the split; a held-out frame then has no neighbours in time")
    return yuvloss.check_flags(args)


def solve_fc_dim(args, final_size, full_data_length):
    """The reference's inline size solver (train_nerv_all.py:193-217): channel width of the stem such that decoder params +
    embedding params ~= --modelsize.  Returns (fc_dim, embed_param) and rewrites args.enc_dim as the reference does."""
    if ('pe' in args.embed or 'le' in args.embed) and "HNeRV_Boost" not in args.model:
        embed_param = 0
        embed_dim = int(args.embed.split('_')[-1]) * 2
        fc_param = np.prod([int(x) for x in args.fc_hw.split('_')])
    else:
        total_enc_strds = np.prod(args.enc_strds)
        embed_hw = final_size / total_enc_strds ** 2
        enc_dim1, embed_ratio = [float(x) for x in args.enc_dim.split('_')]
        embed_dim = int(embed_ratio * args.modelsize * 1e6 / full_data_length / embed_hw) if embed_ratio < 1 else int(embed_ratio)
        embed_param = float(embed_dim) / total_enc_strds ** 2 * final_size * full_data_length
        if args.interpolation:
            embed_param = embed_param / 2
        args.enc_dim = f'{int(enc_dim1)}_{embed_dim}'
        fc_param = (np.prod(args.enc_strds) // np.prod(args.dec_strds)) ** 2 * 9
    decoder_size = args.modelsize * 1e6 - embed_param
    ch_reduce = 1. / args.reduce
    dec_ks1, dec_ks2 = [int(x) for x in args.ks.split('_')[1:]]
    fix_ch_stages = len(args.dec_strds) if args.saturate_stages == -1 else args.saturate_stages
    a = ch_reduce * sum([ch_reduce ** (2 * i) * s ** 2 * min((2 * i + dec_ks1), dec_ks2) ** 2 for i, s in enumerate(args.dec_strds[:fix_ch_stages])])
    b = embed_dim * fc_param
    c = args.lower_width ** 2 * sum([s ** 2 * min(2 * (fix_ch_stages + i) + dec_ks1, dec_ks2) ** 2 for i, s in enumerate(args.dec_strds[fix_ch_stages:])])
    fc_dim = args.fc_dim if args.fc_dim is not None else int(np.roots([a, b, c - decoder_size]).max())
    return fc_dim, embed_param


def build_model(args):
    if args.model == "NeRV_Boost":
        args.expansion = 1
        return NeRV_Boost(1, args=args)
    if args.model == "ENeRV_Boost":
        args.expansion = 3
        return ENeRV_Boost(3, args=args)
    if args.model == "HNeRV_Boost":
        return HNeRV_Boost(args)
    if args.model == "HNeRV":
        return HNeRV(args)
    raise ValueError(f"unknown --model {args.model!r}")


def main(argv=None):
    args = parse_args(argv)
    torch.set_printoptions(precision=2)
    if args.bitstream or args.bitstream_temporal:          # what no file can hold is refused before the run, not after its last epoch
        from .codec import check_posthoc_flags
        check_posthoc_flags(args)
    if args.debug:
        args.eval_freq, args.outf = 1, 'output/debug'
    else:
        args.outf = os.path.join('output', args.outf)
    args.enc_strd_str = ','.join(str(x) for x in args.enc_strds)
    args.dec_strd_str = ','.join(str(x) for x in args.dec_strds)
    args.quant_str = f'quant_M{args.quant_model_bit}_E{args.quant_embed_bit}'
    args.exp_id = f'{args.vid}/Size{args.modelsize}'
    args.outf = os.path.join(args.outf, args.exp_id)
    if args.overwrite and os.path.isdir(args.outf):
        print('Will overwrite the existing output dir!')
        shutil.rmtree(args.outf)
    os.makedirs(args.outf, exist_ok=True)
    args.ngpus_per_node = torch.cuda.device_count()
    env_world = int(os.environ.get("WORLD_SIZE", "1"))
    if env_world > 1:                                      # launched by torchrun: one process per GPU exists already
        args.distributed, args.ngpus_per_node, args.init_method = True, env_world, "env://"
        train(int(os.environ.get("LOCAL_RANK", 0)), args)
    elif args.distributed and args.ngpus_per_node > 1:     # the reference's own launch form: -d spawns one process per GPU
        args.init_method = f'tcp://127.0.0.1:{hash(args.exp_id) % 20000 + 10000}'
        print(f'init_method: {args.init_method}', flush=True)
        mp.spawn(train, nprocs=args.ngpus_per_node, args=(args,))
    else:
        train(None, args)


def data_to_gpu(x, device):
    return x.to(device, non_blocking=True)


_IndexOnly = rt.IndexOnly      # (name kept for the loader-order test)


def _join_process_group(local_rank, args):
    """-> (world, device).  One process per GPU over RCCL; the per-GPU batch is -b / #GPUs as in the reference (:168)."""
    if not (args.distributed and args.ngpus_per_node > 1):
        return 1, torch.device('cuda', local_rank if local_rank is not None else 0)
    rank = int(os.environ["RANK"]) if args.init_method == "env://" else local_rank
    dist.init_process_group(backend='nccl', init_method=args.init_method, world_size=args.ngpus_per_node, rank=rank)
    torch.cuda.set_device(local_rank)
    world = args.ngpus_per_node
    if args.batchSize < world:
        raise ValueError(f"-b {args.batchSize} with {world} GPUs gives a per-GPU batch of 0 (the reference needs -b >= #GPUs)")
    args.batchSize = args.batchSize // world
    return world, torch.device('cuda', local_rank)


def _make_loaders(args, world):
    """Full-clip loader (evaluation, unshuffled) and train loader (shuffled, drop_last) in the reference's construction order --
    the loaders consume the global RNG, and the frame order golden pins it.  With frames resident in HBM the loaders iterate
    indices only."""
    full = VideoDataSet(args)
    args.final_size, args.full_data_length = full.final_size, len(full)
    resident = not args.host_frames and not full.embed_inter
    items = rt.IndexOnly(len(full)) if resident else full
    workers = 0 if resident else args.workers
    sharded = torch.utils.data.distributed.DistributedSampler

    def loader(ds, batch, train):
        sampler = sharded(ds) if world > 1 else None
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=(train and sampler is None), num_workers=workers, pin_memory=True,
                                           sampler=sampler, drop_last=train, worker_init_fn=worker_init_fn)
    full_loader = loader(items, args.batchSize, False)
    train_ids, args.val_ind_list = data_split(list(range(args.full_data_length)), [int(x) for x in args.data_split.split('_')], args.shuffle_data, 0)
    train_loader = loader(Subset(items, train_ids), args.batchSize, True)
    return full, full_loader, train_loader, resident


def _make_optimizer(model, args):
    if args.optim_type == "Adam":
        if args.model == "HNeRV":              # the baseline's recipes: the fused Adam of this package (capturable; torch.optim.Adam's state_dict layout)
            from .optimizer import Adam
            return Adam(model.parameters(), lr=args.lr)
        return optim.Adam(model.parameters(), lr=args.lr)
    if args.optim_type == "Adan":
        from .optimizer import Adan
        return Adan(model.parameters(), lr=args.lr)
    raise ValueError(f"--optim_type {args.optim_type!r}: pass Adan or Adam (the reference's default 'adan' matches neither of its branches)")


def step_mode(optimizer, args):
    """Which train step a run takes: "captured" -- engine.TrainStep, one replayed hipGraph per step (eager under --no_graph) -- for the
    fused optimizers of this package (they have launch_step()), whatever --inpanting mask or --clip_max_norm the recipe sets: the step
    takes the mask and clips on the device.  "generic" -- _generic_step, eager, op by op -- for a stock torch optimizer
    (--optim_type Adam on a boost model).  Needs no GPU."""
    return "captured" if hasattr(optimizer, "launch_step") else "generic"


def train(local_rank, args):
    for seed_fn in (torch.manual_seed, np.random.seed, random.seed):
        seed_fn(args.manualSeed)
    if not torch.cuda.is_available():
        raise RuntimeError("train_nerv_all: no ROCm GPU visible -- the decoder path has no CPU fallback")
    world, device = _join_process_group(local_rank, args)
    is_main = local_rank in (0, None)
    args.metric_names = list(rt.METRIC_NAMES)
    best = rt.BestTracker(args.metric_names)
    log = rt.RunLog(args.outf, is_main)

    full_dataset, full_loader, train_loader, resident = _make_loaders(args, world)
    args.dump_vis = args.dump_images or args.dump_videos
    args.fc_dim, embed_param = solve_fc_dim(args, args.final_size, args.full_data_length)
    model = build_model(args)

    writer = None
    if is_main:
        rt.dump_args(args, args.outf)
        args.encoder_param = sum(p.numel() for p in model.encoder.parameters()) / 1e6
        args.decoder_param = model.decoder_params()
        args.total_param = args.decoder_param + embed_param / 1e6
        sizes = f'Encoder_{round(args.encoder_param, 2)}M_Decoder_{round(args.decoder_param, 4)}M_Total_{round(args.total_param, 4)}M'
        print(f'{args}\n {sizes}', flush=True)
        log.line(f'{model}\n{sizes}', echo=False)
        try:
            from torch.utils.tensorboard import SummaryWriter
            writer = SummaryWriter(os.path.join(args.outf, sizes, 'tensorboard'))
        except Exception:
            writer = None

    print(f"Use GPU: {local_rank} for training")
    model = model.to(device)
    optimizer = _make_optimizer(model, args)
    args.transform_func = TransformInput(args)
    ckpt = rt.load_initial_state(model, args, args.outf, rename=lambda k: k.replace('blocks.0.', '').replace('module.', ''))
    if args.start_epoch < 0:
        args.start_epoch = max(ckpt['epoch'] if ckpt is not None else 0, 0)

    args._frames_dev = full_dataset.to_device(device) if resident else None
    yuv_term = None if args.eval_only else yuvloss.make_term(args, full_dataset, device, resident)

    # pruning (off by default): the masks live in a Pruner; a checkpoint that carries them restores them (resume, --weight, --eval_only)
    pruner = None
    if args.prune_sparsity > 0 or (ckpt is not None and 'prune' in ckpt):
        if not args.eval_only and step_mode(optimizer, args) != "captured":
            raise NotImplementedError("pruning (--prune_sparsity, or a checkpoint with masks) needs the captured train step (Adan, or Adam on the HNeRV baseline): the generic eager step "
                                      "of a stock torch optimizer does not mask its gradients")
        from .prune import Pruner
        pruner = Pruner(model, optimizer)
        if ckpt is not None and 'prune' in ckpt:
            pruner.load_state_dict(ckpt['prune'])
    args._pruner = pruner

    if args.eval_only:
        values, hw = evaluate(model, full_loader, local_rank, args, args.dump_vis, huffman_coding=True)
        top = best.update(values)
        text = f'PSNR for output {hw} for quant {args.quant_str}: ' + ''.join(
            f'best_{n}: {rt.fmt(v, 2 if "psnr" in n else 4)} | ' for n, v in zip(args.metric_names, top))
        if is_main:
            print(text, flush=True)
            with open(os.path.join(args.outf, 'eval.txt'), 'a') as f:
                f.write(text + '\n\n')
            args.train_time, args.cur_epoch = 0, args.epochs
            rt.write_results_csv(args, top, values, [torch.tensor(0)], 'eval.csv')
        return

    h, w = frame_hw(args)
    takes_image = 'pe' not in args.embed or "HNeRV_Boost" in args.model
    mode = step_mode(optimizer, args)                                                 # "captured": Adan, and Adam for the HNeRV baseline
    # the reference's masks depend on the frame size only: built once, on a dummy frame of the crop size (None without --inpanting)
    mask = None if args.transform_func.identity else args.transform_func(torch.zeros(1, 3, h, w, device=device), None)[2]
    step = TrainStep(model, optimizer, args.loss, takes_image, (args.batchSize, 3, h, w), device, use_graph=not args.no_graph,
                     world_size=world, clip_max_norm=args.clip_max_norm, mask=mask, prune=pruner, yuv=yuv_term) if mode == "captured" else None
    # events of this run: those of epochs already trained (resume) are in the checkpoint's masks
    from .prune import schedule as prune_schedule
    prune_events = {e: (j, s) for j, (e, s) in enumerate(prune_schedule(args.prune_sparsity, args.prune_steps))} if args.prune_sparsity > 0 else {}
    log.line(f'Train step: {mode}' + (' (eager: --no_graph)' if mode == "captured" and args.no_graph else '')
             + f', inpainting mask: {args.inpanting if mask is not None else "none"}, clip_max_norm: {args.clip_max_norm}', echo=False)
    if yuv_term is not None:
        log.line(yuvloss.describe(yuv_term, full_dataset.resize), echo=False)
    if full_dataset.resize is not None:
        from .resize import describe as describe_resize
        log.line(describe_resize((full_dataset.crop_h, full_dataset.crop_w), full_dataset.resize), echo=False)
    if args.embed_inter_stored:
        stored, _ = interp_plan(args.full_data_length, args.data_split)
        log.line(f'Interpolation: {len(stored)} of {args.full_data_length} frames stored, {args.full_data_length - len(stored)} derived '
                 f'(split {args.data_split})', echo=False)
    # the generic path (stock Adam) averages its gradients over the ranks with the same flat bucket the fused step uses
    bucket = GradBucket(model.parameters()) if (step is None and world > 1) else None

    t_start = time.time()
    epoch_secs, psnr_trace = [], []
    values = [torch.zeros(1) for _ in args.metric_names]
    lr = args.lr
    for epoch in range(args.start_epoch, args.epochs):
        model.train()
        if epoch in prune_events:
            j, target = prune_events[epoch]
            ev = pruner.prune_to(target)
            pruner.step_index = j
            log.line(f"Prune: epoch {epoch}, target {target:.4f}, pruned {ev['pruned']} of {ev['n']} ({ev['pruned'] / ev['n']:.4f}), threshold {ev['tau']:.6e}",
                     every_rank=False)
        t_epoch = time.time()
        psnr_sum = torch.zeros((), dtype=torch.float32, device=device)     # accumulated on the device: no per-step host sync
        seen = 0
        n_iter = len(train_loader)
        for i, sample in enumerate(train_loader):
            if args.debug and i > 10:
                break
            norm_idx, img_idx = data_to_gpu(sample['norm_idx'], device), data_to_gpu(sample['idx'], device)
            frames = args._frames_dev[img_idx] if resident else data_to_gpu(sample['img'], device)
            lr = adjust_lr(optimizer, (epoch + float(i) / n_iter) / args.epochs, i, args)
            if step is not None:
                _, psnr_b = step(frames, norm_idx) if yuv_term is None else step(frames, norm_idx, frame_idx=img_idx)
                yuv_stats, yuv_ms = step.yuv_stats_out, step.yuv_ms_out
            else:
                psnr_b = _generic_step(model, optimizer, bucket, args, frames, img_idx, norm_idx, takes_image, yuv_term)
                yuv_stats, yuv_ms = getattr(args, '_yuv_stats_out', None), getattr(yuv_term, 'ms_out', None)
            psnr_sum += psnr_b.sum()
            seen += psnr_b.numel()
            if i % args.print_freq == 0 or i == n_iter - 1:                 # the only host sync of the loop
                log.line('[{}] Rank:{}, Epoch[{}/{}], Step [{}/{}], lr:{:.2e} pred_PSNR: {}'.format(
                    log.stamp(), local_rank, epoch + 1, args.epochs, i + 1, n_iter, lr, rt.fmt((psnr_sum / seen).cpu(), 4))
                    + ('' if yuv_term is None else yuvloss.train_text(yuv_term, yuv_stats, yuv_ms)))
        train_psnr = psnr_sum / max(seen, 1)
        if world > 1:
            dist.all_reduce(train_psnr)
            train_psnr /= world
        if is_main:
            now = time.time()
            if writer is not None:
                writer.add_scalar(f'Train/pred_PSNR_{h}X{w}', train_psnr.cpu(), epoch + 1)
                writer.add_scalar('Train/lr', lr, epoch + 1)
            print("Time/epoch: \tCurrent:{:.2f} \tAverage:{:.2f}".format(now - t_epoch, (now - t_start) / (epoch + 1 - args.start_epoch)))
            epoch_secs.append(now - t_epoch)

        last = epoch == args.epochs - 1
        if (epoch + 1) % args.eval_freq == 0 or (args.epochs - epoch) in (1, 3, 5):
            values, hw = evaluate(model, full_loader, local_rank, args, args.dump_vis and last, last)
            if is_main:
                top = best.update(values)
                for name, v, b in zip(args.metric_names, values, top):
                    if 'psnr' in name and writer is not None:
                        writer.add_scalar(f'Val/{name}_{hw}', v.max(), epoch + 1)
                        writer.add_scalar(f'Val/best_{name}_{hw}', b, epoch + 1)
                psnr_trace.append(values[args.metric_names.index('pred_seen_psnr')].max())
                log.line(f'Eval at epoch {epoch + 1} for {hw}: ' + ''.join(f'{n}: {rt.fmt(v, 4)} | ' for n, v in zip(args.metric_names, values)))

        if is_main:
            state = {'epoch': epoch + 1, 'state_dict': model.state_dict(), 'optimizer': optimizer.state_dict()}
            if pruner is not None:
                state['prune'] = pruner.state_dict()
            torch.save(state, os.path.join(args.outf, 'model_latest.pth'))
            if last:
                args.cur_epoch, args.train_time = epoch + 1, rt.hms(time.time() - t_start)
                rt.write_results_csv(args, best.best, values, psnr_trace, f'epoch{epoch + 1}.csv')

    total = float(sum(epoch_secs))
    text = f"Training complete in: {rt.hms(time.time() - t_start)}\n Training wo evaluation complete in: {rt.hms(total)}, {total}s"
    print(text)
    if is_main:
        log.line(text, echo=False)
    if world > 1:
        dist.destroy_process_group()


def _generic_step(model, optimizer, bucket, args, frames, img_idx, norm_idx, takes_image, yuv_term=None):
    """One eager step for the configuration the captured step does not cover (--optim_type Adam on a boost model: torch.optim.Adam), with
    or without an --inpanting mask: the same kernels, driven op by op.  With several ranks the gradients are averaged through the flat bucket before clipping / the step
    (the reference gets this from its DistributedDataParallel wrap).  yuv_term (engine.YuvTerm): lam times the plane loss is added through
    its autograd form (or is the whole loss: --loss YUV420) and its [B, 4] stats are left in args._yuv_stats_out."""
    img_in, img_gt, mask = args.transform_func(frames, img_idx)
    out, _, _ = model(img_in if takes_image else norm_idx, norm_idx=norm_idx)
    yuv_stats = None
    if yuv_term is not None and yuv_term.pure:
        loss, yuv_stats = yuvloss.eager_term(yuv_term, out, img_idx)
    else:
        loss = loss_fn(out, img_gt, args.loss) if mask is None else loss_fn(out * mask, img_gt * mask, args.loss)
        if yuv_term is not None:
            term, yuv_stats = yuvloss.eager_term(yuv_term, out, img_idx)
            loss = loss + term
    optimizer.zero_grad()
    loss.backward()
    if bucket is not None:
        bucket.allreduce_mean()
    if args.clip_max_norm > 0:
        torch.nn.utils.clip_grad_norm_(model.parameters(), args.clip_max_norm)
    optimizer.step()
    if yuv_term is not None:
        args._yuv_stats_out = yuv_stats
    return psnr_fn_device(out.detach(), img_gt)


def _huffman_depths(counts):
    """Code length of every leaf of a Huffman code built over the data symbols (counts, in order) plus one EOF symbol of count 1, the
    last entry of the returned list -- the construction behind _huffman_total_bits, whose depths are the code lengths a qstream file
    stores."""
    n = len(counts)
    heap = [(int(c), i, [i]) for i, c in enumerate(list(counts) + [1])]      # last leaf = EOF
    depth = [0] * (n + 1)
    heapq.heapify(heap)
    uid = n + 1
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        for leaf in a[2] + b[2]:
            depth[leaf] += 1
        heapq.heappush(heap, (a[0] + b[0], uid, a[2] + b[2]))
        uid += 1
    return depth


def _huffman_total_bits(counts):
    """sum_i count_i * code_length_i of a Huffman code built over the data symbols plus one EOF symbol of count 1 -- what
    the reference obtains from dahuffman's HuffmanCodec.from_data + get_code_table (train_nerv_all.py:593-605).  Every optimal
    code has the same total over all leaves; which tie the EOF leaf wins can move the data-only total by a bit or two."""
    return sum(int(c) * d for c, d in zip(counts, _huffman_depths(counts)[:len(counts)]))


def quant_model(model, args):
    """[fp32 copy, post-hoc quantised twin], {key: quantised tensor record} -- the two models evaluate() reports on
    (reference train_nerv_all.py:622-642).  Every decoder tensor goes through hnerv_utils.quant_tensor at --quant_model_bit bits;
    the encoder is left alone (it is not part of the transmitted model).  --quant_model_bit -1 disables the twin.
    --bitstream_sparse: the entries pruning acts on (prune.prunable: dim() > 1) go through quant_tensor_sparse instead, which keeps every
    zero of the tensor -- whoever put it there -- exactly zero; their records carry `keep`."""
    plain = copy.deepcopy(model)
    if args.quant_model_bit == -1:
        return [plain], None
    twin = copy.deepcopy(model)
    records, dequantised = {}, {}
    for key, tensor in twin.state_dict().items():
        if 'encoder' in key:
            dequantised[key] = tensor
        else:
            sparse = getattr(args, 'bitstream_sparse', False) and tensor.dim() > 1
            records[key], dequantised[key] = (quant_tensor_sparse if sparse else quant_tensor)(tensor, args.quant_model_bit)
    twin.load_state_dict(dequantised)
    return [plain, twin], records


def _timed_decodes(net, cur_input, embed, norm_idx, graph):
    """100 repeated decodes of one batch for --eval_fps; a captured hipGraph of the same forward unless BNERV_EVAL_GRAPH=0."""
    times = []
    if cur_input.is_cuda and os.environ.get('BNERV_EVAL_GRAPH', '1') != '0':
        from .engine import DecodeGraph
        if graph is None or not graph.matches(cur_input, embed, norm_idx):
            graph = DecodeGraph(net, cur_input, embed, norm_idx)
        for _ in range(100):
            times.append(graph(cur_input, embed, norm_idx)[1])
    else:
        for _ in range(100):
            times.append(net(cur_input, embed, norm_idx=norm_idx)[2])
    return times, graph


@torch.no_grad()
def _encode_stored(net, full_dataloader, args, frames_dev):
    """[S, C, h, w]: the encoder's embedding of every stored frame of an --embed_inter_stored run (interp_plan's `stored`, in that order), one
    frame per call as the evaluation loop feeds it.  Frames come from the resident clip, or from the loader's dataset under --host_frames."""
    stored = interp_plan(args.full_data_length, args.data_split, args.shuffle_data)[0]
    device = next(net.parameters()).device
    was_training = net.training
    net.eval()
    rows = []
    for k in stored:
        frame = frames_dev[k:k + 1] if frames_dev is not None else data_to_gpu(full_dataloader.dataset[k]['img'][None], device)
        img_in, _gt, _mask = args.transform_func(frame, torch.tensor([k], device=device))
        rows.append(net.forward_encoder(img_in))
    net.train(was_training)
    return torch.cat(rows, 0).contiguous()


@torch.no_grad()
def evaluate(model, full_dataloader, local_rank, args, dump_vis=False, huffman_coding=False):
    """PSNR / MS-SSIM of the fp32 model and of its post-hoc quantised twin over the whole clip (seen / unseen frames apart),
    decode FPS, and -- on request -- the Huffman bit accounting of the quantised tensors.  Returns (values per metric slot, (h, w))."""
    nets, records = quant_model(model, args)
    book = rt.MetricBook(args.val_ind_list, args.metric_names)
    log = rt.RunLog(args.outf, local_rank in (0, None))
    frames_dev = getattr(args, '_frames_dev', None)
    takes_image = 'pe' not in args.embed or "HNeRV_Boost" in args.model
    is_hnerv = "HNeRV" in args.model
    embeds, dequant_embeds, quant_embed = [], None, None
    fps, hw = 0.0, (0, 0)
    # --embed_inter_stored: the encoder runs over the stored frames only; every frame's embedding, in both slots, is a row
    # of ops.embed_expand over that table (fp32 slot) or over its de-quantised twin (quantised slot: what a decoder of the file holds)
    from_stored = getattr(args, 'embed_inter_stored', False) and is_hnerv
    if from_stored:
        plan = interp_plan(args.full_data_length, args.data_split, args.shuffle_data)[1]
        stored_table = _encode_stored(nets[0], full_dataloader, args, frames_dev)
        quant_embed, deq = quant_tensor(stored_table, args.quant_embed_bit)
        expanded = [ops.embed_expand(stored_table, plan), ops.embed_expand(deq.float().contiguous(), plan)]
    for slot, net in enumerate(nets):
        net.eval()
        net.time_decode = True
        device = next(net.parameters()).device
        times, graph = [], None
        vis_dir = None
        if dump_vis:
            vis_dir = os.path.join(args.outf, 'visualize_model' + ('_quant' if slot else '_orig'))
            os.makedirs(vis_dir, exist_ok=True)
        n_batches = len(full_dataloader)
        for i, sample in enumerate(full_dataloader):
            if args.debug and i > 10:
                break
            norm_idx, img_idx = data_to_gpu(sample['norm_idx'], device), data_to_gpu(sample['idx'], device)
            frames = frames_dev[img_idx] if frames_dev is not None else data_to_gpu(sample['img'], device)
            img_in, img_gt, _mask = args.transform_func(frames, img_idx)
            cur_input = img_in if takes_image else norm_idx
            if from_stored:
                embed_in = expanded[slot][img_idx]
            else:
                embed_in = dequant_embeds[i] if (slot and is_hnerv) else None
            extra = {}
            if args.interpolation and args.embed_inter and 'pre_img' in sample and img_idx.item() in args.val_ind_list:
                extra = dict(pre_img=data_to_gpu(sample['pre_img'], device), post_img=data_to_gpu(sample['post_img'], device))
            out, embed_list, dec_time = net(cur_input, embed_in, norm_idx=norm_idx, **extra)
            if slot == 0 and not from_stored:
                embeds.append(embed_list[0])
            if args.eval_fps:
                more, graph = _timed_decodes(net, cur_input, embed_list[0], norm_idx, graph)
                times.extend(more)
            else:
                times.append(dec_time)
            psnr, ssim = ops.psnr(out, img_gt), ops.msssim(out.float(), img_gt)     # stay on the device until a line is printed
            book.add(slot, sample['idx'].tolist(), psnr, ssim)
            if dump_vis:
                _save_images(out, psnr, vis_dir, i, args)
            if i % args.print_freq == 0 or i == n_batches - 1:
                fps = args.batchSize / (sum(times) / len(times))
                log.line(f'[{log.stamp()}] Rank:{local_rank}, Eval at Step [{i + 1}/{n_batches}] , FPS {round(fps, 1)}, ' + book.describe(book.running()),
                         every_rank=False)
        if slot == 0 and is_hnerv and not from_stored:
            quant_embed, deq = quant_tensor(torch.cat(embeds, 0), args.quant_embed_bit)
            dequant_embeds = deq.split(args.batchSize, dim=0)
        args.fps, hw = fps, tuple(frames.shape[-2:])
        net.time_decode = False
        net.train()
    values = book.means(device=next(model.parameters()).device)
    if local_rank in (0, None) and records is not None and huffman_coding:
        _huffman_report(args, records, quant_embed if is_hnerv else None, log)
        pruner = getattr(args, '_pruner', None)
        if pruner is not None:
            log.line(f'Sparsity: {pruner.pruned()} of {pruner.n} prunable weights are zero ({pruner.sparsity():.4f})')
    if local_rank in (0, None) and huffman_coding and getattr(args, 'bitstream', None):
        from . import codec
        args.bitstream_budget = codec.encode_posthoc(model, args, records, quant_embed if is_hnerv else None, args.bitstream,
                                                     temporal=getattr(args, 'bitstream_temporal', False))
        log.line(f'Bitstream {args.bitstream}: {codec.describe_any(args.bitstream_budget)}')
    return values, hw


def _huffman_report(args, records, quant_embed, log):
    """Bits per parameter / per pixel of the post-hoc quantised tensors under one Huffman code over all symbols, plus 16 bits for
    every stored (min, scale) entry (reference train_nerv_all.py:577-612)."""
    symbols, side_entries = [], 0
    recs = ([quant_embed] if quant_embed is not None else []) + list(records.values())
    for rec in recs:
        symbols.append(rec['quant'].flatten().cpu())
        side_entries += rec['min'].nelement() + rec['scale'].nelement()
    flat = torch.cat(symbols).to(torch.int64)
    if any('keep' in rec for rec in recs):                 # --bitstream_sparse: the bits of the parsed leaves, zero runs among them
        from . import codec
        bits = codec.sparse_code(*codec.posthoc_symbols(recs))[2]
    else:
        hist = torch.bincount(flat, minlength=1)
        bits = _huffman_total_bits(hist[hist > 0].tolist())
    args.bits_per_param = bits / flat.numel()
    bits += side_entries * 16
    args.full_bits_per_param = bits / flat.numel()
    args.total_bpp = bits / args.final_size / args.full_data_length
    log.line(f'After quantization and encoding: \n bits per parameter: {round(args.full_bits_per_param, 2)}, bits per pixel: {round(args.total_bpp, 4)}')


def _save_images(out, psnr, vis_dir, batch_no, args):
    from PIL import Image
    for b in range(out.shape[0]):
        arr = (out[b].clamp(0, 1) * 255 + 0.5).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
        Image.fromarray(arr).save(os.path.join(vis_dir, f'pred_{batch_no * args.batchSize + b:04d}_{round(psnr[b].item(), 2)}.png'))


Dump2CSV = rt.write_results_csv      # (the reference's name for the results table writer)


if __name__ == '__main__':
    main()
