from .dla import DLA, DLABackbone, dla34, build_dla_from_vision_fpn_backbone
from .fpn import FPN, Backbone, to_channels_last
from .fpn import LastLevelMaxPool
from .resnet import ResNet, build_resnet_from_vision_fpn_backbone
from .densenet import DenseNetBackbone, build_densenet_fpn_backbone
from .shufflenet import ShufflenetBackbone, build_shufflenet_fpn_backbone
from .mnasnet import MNASNetBackbone, build_mnasnet_fpn_backbone
