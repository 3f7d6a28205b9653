"""The option-critic family (reference `algorithm/oc/`).  So far: `OptionBase`, the learner of one option."""
from .option_base import OptionBase  # noqa: F401
