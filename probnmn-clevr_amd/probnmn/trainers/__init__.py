"""The training iterations.  Each lives in its own module; ``MarginalJointStep``, ``ImportanceWeightedCodingStep`` and
``ImportanceWeightedJointStep`` are also reachable from here (resolved on first use, so importing the package stays as cheap
as it was)."""

__all__ = ["MarginalJointStep", "ImportanceWeightedCodingStep", "ImportanceWeightedJointStep"]


def __getattr__(name):
    if name == "MarginalJointStep":
        from .marginal_training import MarginalJointStep

        return MarginalJointStep
    if name == "ImportanceWeightedCodingStep":
        from .importance_weighted import ImportanceWeightedCodingStep

        return ImportanceWeightedCodingStep
    if name == "ImportanceWeightedJointStep":
        from .importance_weighted import ImportanceWeightedJointStep

        return ImportanceWeightedJointStep
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
