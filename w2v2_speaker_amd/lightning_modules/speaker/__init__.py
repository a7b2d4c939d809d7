from .xvector import XVectorModule, XVectorModuleConfig  # noqa: F401
