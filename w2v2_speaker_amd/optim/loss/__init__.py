from .aam_softmax import AngularAdditiveMarginSoftMaxLoss  # noqa: F401
from .binary_cross_entropy import BinaryCrossEntropyLoss  # noqa: F401
from .cross_entropy import CrossEntropyLoss  # noqa: F401
from .ctc_loss import CtcLoss  # noqa: F401
from .triplet_loss import TripletLoss  # noqa: F401
from .triplet_ce_loss import TripletCrossEntropyLoss  # noqa: F401
from .margin_softmax import SubCenterMarginSoftMaxLoss  # noqa: F401
