from .config import OptimConfig  # noqa: F401
