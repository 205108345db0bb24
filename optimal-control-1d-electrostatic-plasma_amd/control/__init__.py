from .actuator import E_field
from .reward import Reward
from .policy import MLPPolicy
from .actor import ParticleActor
