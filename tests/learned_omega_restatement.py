"""NumPy restatement of the learned MMA iterations with one omega per layer (iterations(..., omega_vec) of the reference's
bdd_cuda_learned_mma<REAL>; bdd_cuda_parallel_mma.cu:45-57,117-128): the deferred difference of layer l is omega[l] * (m1 - m0), one product
in REAL as in LearnedMma._layer_mm.  omega is indexed like the layers of LearnedMma: BDD-major order.  Test helper only."""
import numpy as np

from learned_mma_restatement import LearnedMma


class LearnedOmegaMma(LearnedMma):
    """LearnedMma whose passes take omega as an array of n_layers values (BDD-major order); a scalar omega still works as before"""

    def _layer_mm(self, l, omega):
        return super()._layer_mm(l, omega[l] if np.ndim(omega) else omega)

    def forward_pass(self, omega, dlo, dhi):
        super().forward_pass(self._omega(omega), dlo, dhi)

    def backward_pass(self, omega, dlo, dhi):
        super().backward_pass(self._omega(omega), dlo, dhi)

    def _omega(self, omega):
        if np.ndim(omega) == 0:
            return omega
        w = np.asarray(omega, self.dt)
        assert w.shape == (self.n_layers,), (w.shape, self.n_layers)
        return w
