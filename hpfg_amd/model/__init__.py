from .builder import build_model
from .segformer import SegFormer, SegFormer_Plus
from .swin import BasicBlock, Mlp, PatchMerging, SwinTransformerBlock, WindowAttention
from .swin_mae import SwinMAE, swin_mae
from .swinunet import (BasicBlockUp, FinalPatchExpanding, PatchEmbedding, PatchExpanding, SwinUnet, SwinUnet_Plus, SwinUnetDecoder, SwinUnetEncoder,
                       get_swinunet, get_swinunet_LIDC, get_swinunet_plus)
from .unet import UNet, UNet_Plus, reset_dropout_streams
from .uniformer import Attention, CBlock, CMlp, PatchEmbed, SABlock, UniFormer, Uniformer_Plus, uniformer_small
from .uniformer import Mlp as UniFormerMlp          # (`Mlp` is the Swin block's, model/swin.py; the classes differ: this one has no dropout)
