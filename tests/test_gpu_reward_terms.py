"""Every post-physics reward term, the termination, the episode sums and the extras of the HIP
post-physics kernel (lgx_envlogic.hip, launched as lgx_step does: with the Go1 actuator net in the
launch where the task has one) against the float64 reference of tests/reward_terms_ref.py - the
body of tests/test_reward_terms.py on the lgx backend, plus the instantiations with a privileged
row and with an observation history."""
import pytest

import reward_terms_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(R.CASES))
def test_reward_terms_match_float64_reference(gpu, name):
    R.run_case(name, device="cuda:0", backend="lgx")
