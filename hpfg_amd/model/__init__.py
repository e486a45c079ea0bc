from .builder import build_model
from .segformer import SegFormer, SegFormer_Plus
from .unet import UNet, UNet_Plus, reset_dropout_streams
