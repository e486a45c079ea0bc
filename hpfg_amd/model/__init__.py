from .builder import build_model
from .segformer import SegFormer, SegFormer_Plus
from .swin import BasicBlock, Mlp, PatchMerging, SwinTransformerBlock, WindowAttention
from .unet import UNet, UNet_Plus, reset_dropout_streams
