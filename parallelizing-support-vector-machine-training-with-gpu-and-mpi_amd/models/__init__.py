"""Estimators and model persistence."""
from .multiclass import OneVsRestSVC
from .ovo import OneVsOneSVC
from .svc import SVC

__all__ = ["SVC", "OneVsRestSVC", "OneVsOneSVC"]
