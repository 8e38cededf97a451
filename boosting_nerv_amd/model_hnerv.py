"""HNeRV (the baseline, model_hnerv.py:11-175) and HNeRV_Boost (model_hnerv.py:178-322) -- host-side mirrors of the reference's classes.
Encoder, decoder and head run on the HIP kernels through ``ops``."""
import time

import torch
import torch.nn as nn

from .model_blocks import *  # noqa: F401,F403
from .model_blocks import ConvNeXt, CustomConv2d, NeRV_MLP, NeRVBlock, PositionEncoding, head_out
from .lib.transform_ops import quant_map
from .model_nerv import _CEMHooks, decoder_layers_forward


class HNeRV(nn.Module):
    """The baseline the boosted models start from (reference model_hnerv.py:11-158), encoder form: ConvNeXt content encoder ->
    decoder[0] (1x1 conv + GELU) -> up-conv blocks (conv k = min(1 + 2 i, 5) + PixelShuffle + GELU, no TAT) -> 3x3 head + tanh.
    Same constructor calls in the same order as the reference, so a seeded init gives the same parameters and state_dict keys."""

    def __init__(self, args):
        super().__init__()
        self.embed = args.embed
        ks_enc, ks_dec1, ks_dec2 = [int(x) for x in args.ks.split("_")]
        enc_blks = args.enc_blks
        if not len(args.enc_strds):
            raise NotImplementedError("HNeRV with enc_strds == [] (the positional-embedding form, model_hnerv.py:36-40) is not on the HIP path")
        if args.conv_type[0] != "convnext":
            raise NotImplementedError(f"HNeRV with conv_type[0]={args.conv_type[0]!r} (the NeRVBlock encoder, model_hnerv.py:27-32) is not on the "
                                      "HIP path: pass --conv_type convnext pshuffel")
        if getattr(args, "quant", False):
            raise NotImplementedError("HNeRV with args.quant (the embedding quantiser of the compression recipe, model_hnerv.py:61-63) is not on the HIP path")
        enc_dim1, enc_dim2 = [int(x) for x in args.enc_dim.split("_")]
        c_out_list = [enc_dim1] * len(args.enc_strds)
        c_out_list[-1] = enc_dim2
        self.encoder = ConvNeXt(stage_blocks=enc_blks, strds=args.enc_strds, dims=c_out_list, drop_path_rate=0)
        hnerv_hw = int(np.prod(args.enc_strds) // np.prod(args.dec_strds))
        self.fc_h, self.fc_w = hnerv_hw, hnerv_hw

        decoder_layers = []
        ngf = args.fc_dim
        out_f = int(ngf * self.fc_h * self.fc_w)
        decoder_layers.append(NeRVBlock(dec_block=False, conv_type="conv", ngf=enc_dim2, new_ngf=out_f, ks=0, strd=1, bias=True,
                                        norm=args.norm, act=args.act, sft_ngf=args.ch_t, args=args))
        for i, strd in enumerate(args.dec_strds):
            reduction = sqrt(strd) if args.reduce == -1 else args.reduce
            new_ngf = int(max(round(ngf / reduction), args.lower_width))
            for j in range(args.dec_blks[i]):
                decoder_layers.append(NeRVBlock(dec_block=True, conv_type=args.conv_type[1], ngf=ngf, new_ngf=new_ngf,
                                                ks=min(ks_dec1 + 2 * i, ks_dec2), strd=1 if j else strd, bias=True, norm=args.norm,
                                                act=args.act, sft_ngf=args.ch_t, args=args))
                ngf = new_ngf
        self.decoder = nn.ModuleList(decoder_layers)
        self.head_layer = CustomConv2d(ngf, 3, 3, 1, 1, args=args)
        self.out_bias = args.out_bias
        self.embed_quantizer = None
        self.time_decode = False

    def _decode(self, img_embed):
        embed_list = [img_embed]
        dec_start = time.time()
        output = _fc_reshape(self.decoder[0](img_embed), self.fc_h, self.fc_w)
        embed_list.append(output)
        for layer in self.decoder[1:]:
            output = layer(output)
            embed_list.append(output)
        img_out = head_out(self.head_layer, output, self.out_bias)
        if self.time_decode and torch.cuda.is_available():
            torch.cuda.synchronize()
        return img_out, embed_list, time.time() - dec_start

    def forward(self, input, input_embed=None, entropy_model=None, pre_img=None, post_img=None, norm_idx=None):
        img_embed = input_embed if input_embed is not None else self.encoder(input)
        if pre_img is not None and post_img is not None:
            img_embed = 0.5 * (self.encoder(pre_img) + self.encoder(post_img))
        return self._decode(img_embed)

    def forward_encoder(self, input):
        return self.encoder(input)

    def forward_decoder(self, img_embed, norm_idx=None):
        return self._decode(img_embed)

    def decoder_params(self):
        return (sum([p.data.nelement() for p in self.parameters()]) - sum([p.data.nelement() for p in self.encoder.parameters()])) / 1e6


def _fc_reshape(output, fc_h, fc_w):
    """model_hnerv.py:87-88: [n, c fc_h fc_w, h, w] -> [n, c, fc_h h, fc_w w]; the identity for fc_h = fc_w = 1 (every encoder recipe)."""
    if fc_h == 1 and fc_w == 1:
        return output
    n, c, h, w = output.shape
    return output.view(n, -1, fc_h, fc_w, h, w).permute(0, 1, 4, 2, 5, 3).reshape(n, -1, fc_h * h, fc_w * w)


class HNeRVDecoder(nn.Module):
    """reference model_hnerv.py:160-175: the decoder and head of a trained HNeRV as a module of their own."""

    def __init__(self, model):
        super().__init__()
        self.fc_h, self.fc_w = [torch.tensor(x) for x in [model.fc_h, model.fc_w]]
        self.out_bias = model.out_bias
        self.decoder = model.decoder
        self.head_layer = model.head_layer

    def forward(self, img_embed):
        output = _fc_reshape(self.decoder[0](img_embed), int(self.fc_h), int(self.fc_w))
        for layer in self.decoder[1:]:
            output = layer(output)
        return head_out(self.head_layer, output, self.out_bias)


class HNeRV_Boost(_CEMHooks, nn.Module):
    lazy_flush_ok = True     # (engine.TrainStep: deferred slab reductions are flushed by their first reader; all readers are this package's operators)
    def __init__(self, args):
        super().__init__()
        self.embed = args.embed
        ks_enc, ks_dec1, ks_dec2 = [int(x) for x in args.ks.split("_")]
        enc_blks = args.enc_blks
        enc_dim1, enc_dim2 = [int(x) for x in args.enc_dim.split("_")]
        c_out_list = [enc_dim1] * len(args.enc_strds)
        c_out_list[-1] = enc_dim2
        self.encoder = ConvNeXt(stage_blocks=enc_blks, strds=args.enc_strds, dims=c_out_list, drop_path_rate=0)

        self.pe_embed_t = PositionEncoding(args.embed, args.lfreq)
        mlp_dim_list = [int(self.pe_embed_t.embed_length)] + [int(args.ch_t * 2)] + [args.ch_t]
        self.stem_t = NeRV_MLP(dim_list=mlp_dim_list, bias=True, act=args.act, omega=1, args=args)

        decoder_layers = []
        ngf = args.fc_dim
        decoder_layers.append(NeRVBlock(dec_block=False, conv_type="conv", ngf=enc_dim2, new_ngf=ngf, ks=0, strd=1, bias=True,
                                        norm=args.norm, act=args.act, sft_ngf=args.ch_t, args=args))
        for i, strd in enumerate(args.dec_strds):
            reduction = sqrt(strd) if args.reduce == -1 else args.reduce
            new_ngf = int(max(round(ngf / reduction), args.lower_width))
            for j in range(args.dec_blks[i]):
                decoder_layers.append(NeRVBlock(dec_block=True, conv_type=args.conv_type[1], ngf=ngf, new_ngf=new_ngf,
                                                ks=min(ks_dec1 + 2 * i, ks_dec2), strd=1 if j else strd, bias=True, norm=args.norm,
                                                act=args.act, sft_ngf=args.ch_t, args=args))
                ngf = new_ngf
        self.decoder = nn.ModuleList(decoder_layers)
        self.head_layer = CustomConv2d(ngf, 3, 3, 1, 1, args=args)
        self.out_bias = args.out_bias
        if args.quant:                                         # model_hnerv.py:216-220
            self.embed_quantizer = quant_map[args.quantizer_e](args.quant_embed_bit, signed=False, per_channel=args.per_channel_e)
            self.bitrate_e_dict = {}
        else:
            self.embed_quantizer = None
        self.outf = args.outf
        self.time_decode = False

    def _decode(self, img_embed, norm_idx):
        embed_list = [img_embed]
        dec_start = time.time()
        # norm_idx arrives as float64 from the loader: the PE product and sin/cos are evaluated in fp64 and cast (:241)
        t_embed = self.stem_t(self.pe_embed_t(norm_idx[:, None]).float())
        output = decoder_layers_forward(self.decoder, img_embed, t_embed, embed_list)
        img_out = head_out(self.head_layer, output, self.out_bias)
        if self.time_decode and torch.cuda.is_available():
            torch.cuda.synchronize()
        return img_out, embed_list, time.time() - dec_start

    def forward(self, input, input_embed=None, entropy_model=None, pre_img=None, post_img=None, norm_idx=None):
        img_embed = input_embed if input_embed is not None else self.encoder(input)
        if self.embed_quantizer is not None:                   # model_hnerv.py:230-234
            self.embed_quantizer.init_data(img_embed)
            code_e, quant_e, img_embed = self.embed_quantizer(img_embed)
            if entropy_model is not None:
                self.bitrate_e_dict.update(entropy_model.cal_bitrate(code_e, quant_e, self.training))
        if pre_img is not None and post_img is not None:
            img_embed = 0.5 * (self.encoder(pre_img) + self.encoder(post_img))
        return self._decode(img_embed, norm_idx)

    def forward_encoder(self, input):
        return self.encoder(input)

    def forward_embed_quant(self, img_embed, entropy_model=None):      # model_hnerv.py:256-260
        code, quant, img_embed = self.embed_quantizer(img_embed)
        if entropy_model is not None:
            self.bitrate_e_dict.update(entropy_model.cal_bitrate(code, quant, self.training))
        return code, quant, img_embed

    def forward_decoder(self, img_embed, norm_idx):
        return self._decode(img_embed, norm_idx)

    def decoder_params(self):
        return (sum([p.data.nelement() for p in self.parameters()]) - sum([p.data.nelement() for p in self.encoder.parameters()])) / 1e6
