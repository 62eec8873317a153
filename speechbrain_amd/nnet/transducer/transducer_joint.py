"""speechbrain.nnet.transducer.transducer_joint mirror (nnet/transducer/transducer_joint.py:61-102)."""
import torch

from speechbrain_amd import native

_ACTS = {torch.nn.GELU: native.ACT_GELU, torch.nn.LeakyReLU: native.ACT_LEAKY_RELU, torch.nn.Tanh: native.ACT_TANH,
         torch.nn.ReLU: native.ACT_RELU}


class Transducer_joint(torch.nn.Module):
    """joint="sum": act(input_TN + input_PN).  The joint runs inside sbk_transducer_greedy_f32 (decoders/transducer.py);
    ``act_code`` names its nonlinearity there.  ``joint="concat"`` and a ``joint_network`` are not implemented."""

    def __init__(self, joint_network=None, joint="sum", nonlinearity=torch.nn.LeakyReLU):
        super().__init__()
        if joint != "sum":
            raise NotImplementedError(f'Transducer_joint(joint="{joint}") is not implemented (only joint="sum")')
        if joint_network is not None:
            raise NotImplementedError("Transducer_joint with a joint_network is not implemented")
        self.joint_network = joint_network
        self.joint = joint
        self.nonlinearity = nonlinearity()

    @property
    def act_code(self):
        nl = self.nonlinearity
        code = _ACTS.get(type(nl))
        if code is None:
            raise NotImplementedError(f"transducer joint nonlinearity {type(nl).__name__} is not implemented")
        if isinstance(nl, torch.nn.GELU) and nl.approximate != "none":
            raise NotImplementedError("GELU(approximate='tanh') in the transducer joint is not implemented")
        if isinstance(nl, torch.nn.LeakyReLU) and nl.negative_slope != 0.01:
            raise NotImplementedError(f"LeakyReLU(negative_slope={nl.negative_slope}) in the transducer joint is not implemented")
        return code

    def forward(self, input_TN, input_PN):
        raise NotImplementedError("Transducer_joint runs inside the transducer search (sbk_transducer_greedy_f32)")
