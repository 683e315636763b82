"""Prototype-namespace mirrors (torchao/prototype/*) that sit on the SURVEY.md section 8 path."""
from .blockwise_fp8 import Float8BlockwiseExpertWeights, fp8_blockwise_grouped_mm  # noqa: F401

__all__ = ["Float8BlockwiseExpertWeights", "fp8_blockwise_grouped_mm"]
