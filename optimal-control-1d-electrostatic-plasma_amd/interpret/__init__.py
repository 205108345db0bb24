from .spectrum import compute_E_k_spectrum
from .landau import (compute_bounce_time, compute_linear_damping_rate, compute_linear_damping_rate_analytic,
                     compute_numerical_entropy, damping_rate, E_k_spectrum)
from ..env.record import Record
