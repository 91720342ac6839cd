"""Encoder registry (same names as reference src/encoder/__init__.py:11-20)."""
from . import pointnet, pointnetpp, voxels
from ..layers import Resnet18, Resnet34, Resnet50, TactileUNet

encoder_dict = {
    'pointnet_local_pool': pointnet.LocalPoolPointnet,
    'voxel_simple_local': voxels.LocalVoxelEncoder,
    'pointnet_plus_plus': pointnetpp.PointNetPlusPlus,
    'UNet': TactileUNet,
    'Resnet18': Resnet18,
    'Resnet34': Resnet34,
    'Resnet50': Resnet50,
}
