"""Model plugin of one option with the GRU representation of `nn_rnn` plus the termination head (the names an option
reads of the reference's `envs/test/nn_rnn.py`)."""
import algorithm.nn_models as m

from .nn_rnn import ModelPolicy, ModelQ, ModelRep  # noqa: F401

ModelTermination = m.ModelTermination
