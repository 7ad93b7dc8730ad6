from .train_and_eval import train_one_epoch, evaluate, create_lr_scheduler, criterion  # noqa: F401
from .distributed_utils import init_distributed_mode, ConfusionMatrix, DiceCoefficient  # noqa: F401
from .boundary_loss import BoundaryLoss, signed_distance2, distance_maps  # noqa: F401
from .lovasz_loss import LovaszSoftmax, sort_pairs, lovasz_errors, lovasz_coefs  # noqa: F401
from .lovasz_loss import LovaszHinge, hinge_errors, hinge_coefs  # noqa: F401
from .distill_loss import Distill, ModelTeacher, EnsembleTeacher  # noqa: F401
