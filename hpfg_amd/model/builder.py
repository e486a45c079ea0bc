"""``build_model(args)``: the reference's string-keyed model factory (model/builder.py:14-62) for the hot-path architectures.

Keys handled here: "unet" -> UNet, "unet_plus" -> UNet_Plus ("unet_lidc" is the same graph in the reference: model/unet_LIDC.py
differs from model/unet.py by whitespace only), "segformer" -> SegFormer-B0, "segformer_plus" -> SegFormer_Plus (MiT-B1 + the projection necks; see model/segformer.py),
"swinunet_plus" -> get_swinunet_plus(img_size=train_crop_size[0]) (Swin-UNet + the projection necks, the key of the reference's
config/ccnet_swinunet_30k_224x224_ACDC.yaml; see model/swinunet.py; "swinunet" itself is still refused), "swinunet_lidc" ->
get_swinunet_LIDC(img_size=train_crop_size[0] or train_crop_size) (the patch-2 Swin-UNet of the reference's model/swinunet_LIDC.py, window 3 at
96 x 96 or 4 at 64 x 64, on the packed small-window attention kernels; the key of config/swinunet_30k_96x96_LIDC.yaml), "swinmae" ->
swin_mae(in_channels, mask_ratio=args.mask_ratio) (the masked-autoencoder pretraining of the Swin encoder, the key of the reference's
config/swinmae_30k_224x224_ACDC.yaml; see model/swin_mae.py), "uniformer_plus" -> Uniformer_Plus (UniFormer-S + SegFormerHead + the projection
necks, the key of the reference's config/ccnet_uniformer_30k_224x224_ACDC.yaml; square inputs with a side of 128 to 256, a multiple of 32;
see model/uniformer.py).  Every other key of the reference's factory is outside this build's scope and
raises NotImplementedError exactly like an unknown key does there (builder.py:59-60).
"""
from .segformer import SegFormer, SegFormer_Plus
from .swin_mae import swin_mae
from .swinunet import get_swinunet_LIDC, get_swinunet_plus
from .unet import UNet, UNet_Plus
from .uniformer import Uniformer_Plus


def build_model(args):
    if args.model in ("unet", "unet_lidc"):
        return UNet(in_channels=args.in_channels, num_classes=args.num_classes)
    if args.model == "unet_plus":
        return UNet_Plus(in_channels=args.in_channels, num_classes=args.num_classes)
    if args.model == "segformer":
        return SegFormer(image_size=args.train_crop_size, in_channels=args.in_channels, num_classes=args.num_classes)
    if args.model == "segformer_plus":
        return SegFormer_Plus(image_size=args.train_crop_size, in_channels=args.in_channels, num_classes=args.num_classes)
    if args.model == "swinunet_plus":
        return get_swinunet_plus(img_size=int(args.train_crop_size[0]), in_channels=args.in_channels, num_classes=args.num_classes)
    if args.model == "swinunet_lidc":          # reference model/builder.py:41-46
        crop = args.train_crop_size
        return get_swinunet_LIDC(img_size=int(crop[0] if isinstance(crop, (list, tuple)) else crop), in_channels=args.in_channels,
                                 num_classes=args.num_classes)
    if args.model == "swinmae":
        return swin_mae(in_channels=args.in_channels, mask_ratio=args.mask_ratio)
    if args.model == "uniformer_plus":          # reference model/builder.py:57-58
        return Uniformer_Plus(image_size=args.train_crop_size, in_channels=args.in_channels, num_classes=args.num_classes)
    raise NotImplementedError(f"model '{args.model}' is outside the MI355X hot-path build (see DESIGN.md, scope)")
