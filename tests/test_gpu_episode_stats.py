"""GPU: lgx_episode_stats_step (through EpisodeStats) against rsl_rl's torch / deque block
(episode_stats_ref.DequeStats, evaluated on the CPU: the bookkeeping is one float32 add per env,
so the comparison is exact - torch.equal on the running sums, == on the deque lists)."""
import ctypes as C

import pytest
import torch

from episode_stats_ref import DequeStats, random_sequence

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1024, 1025, 4096]    # across the wave (64) and the tile (1024) boundary


def make_pair(n, cap, count0, gpu, seed=0):
    """EpisodeStats on the GPU and the deque reference in the same state: random running sums and
    `count0` episodes already recorded (the last min(count0, cap) of them still held)."""
    from legged_gym_amd.rl.episode_stats import EpisodeStats
    g = torch.Generator().manual_seed(seed)
    st, ref = EpisodeStats(n, gpu, capacity=cap), DequeStats(n, "cpu", capacity=cap)
    assert st.on_device
    ref.cur_reward_sum.copy_(torch.randn(n, generator=g))
    ref.cur_episode_length.copy_(torch.randint(0, 1000, (n,), generator=g).float())
    st.cur_sum.copy_(ref.cur_reward_sum)
    st.cur_len.copy_(ref.cur_episode_length)
    held = min(count0, cap)
    hist = torch.randn(2, held, generator=g)
    rings = torch.zeros(2, cap)
    for i in range(held):
        rings[:, (count0 - held + i) % cap] = hist[:, i]
    st.rings.copy_(rings)
    st.count.fill_(count0)
    ref.rewbuffer.extend(hist[0].tolist())
    ref.lenbuffer.extend(hist[1].tolist())
    return st, ref


def check_step(st, ref, rew, dones, gpu, what=""):
    before = int(st.count.item())
    ref.step(rew, dones)
    st.step(rew.to(gpu), dones.to(gpu))
    st.request()
    assert torch.equal(st.cur_sum.cpu(), ref.cur_reward_sum), what
    assert torch.equal(st.cur_len.cpu(), ref.cur_episode_length), what
    assert st.result() == ref.lists(), what
    assert int(st.count.item()) == before + int(dones.sum()), what


def patterns(n, cap):
    spread = lambda k: [i * (n - 1) // (k - 1) for i in range(k)]   # k <= n distinct envs, first and last included
    out = {"none": [], "env 0": [0], "last env": [n - 1], "all": list(range(n))}
    if n >= cap:
        out["capacity"] = spread(cap)
    if n >= cap + 1:
        out["capacity + 1"] = spread(cap + 1)
    return out


@pytest.mark.parametrize("cap", [100, 7])
@pytest.mark.parametrize("n", SIZES)
def test_single_step_patterns(gpu, n, cap):
    for i, (name, ids) in enumerate(patterns(n, cap).items()):
        assert len(set(ids)) == len(ids)
        st, ref = make_pair(n, cap, count0=5, gpu=gpu, seed=i)
        dones = torch.zeros(n, dtype=torch.bool)
        dones[ids] = True
        rew = torch.randn(n, generator=torch.Generator().manual_seed(100 + i))
        check_step(st, ref, rew, dones, gpu, name)


@pytest.mark.parametrize("cap", [100, 7])
@pytest.mark.parametrize("count0", ["cap - 3", 2 ** 31 - 3, 2 ** 31 + 1, 2 ** 32 - 2])
def test_ring_wrap(gpu, cap, count0):
    """5 envs finish 3 slots before the end of the ring; and with count around 2^31 / 2^32 (64-bit
    slot arithmetic)."""
    n = 1025
    if count0 == "cap - 3":
        count0 = 3 * cap + cap - 3
        assert count0 % cap == cap - 3
    st, ref = make_pair(n, cap, count0, gpu)
    dones = torch.zeros(n, dtype=torch.bool)
    dones[[3, 64, 500, 1023, 1024]] = True
    check_step(st, ref, torch.randn(n, generator=torch.Generator().manual_seed(1)), dones, gpu)
    dones = torch.zeros(n, dtype=torch.bool)
    dones[[0, 63, 1024]] = True
    check_step(st, ref, torch.randn(n, generator=torch.Generator().manual_seed(2)), dones, gpu)


def test_random_sequence_and_determinism(gpu):
    from legged_gym_amd.rl.episode_stats import EpisodeStats
    seq = random_sequence()
    n = seq[0][0].numel()
    st, ref = EpisodeStats(n, gpu), DequeStats(n, "cpu")
    for t, (rew, dones) in enumerate(seq):
        check_step(st, ref, rew, dones, gpu, t)
    again = EpisodeStats(n, gpu)
    for rew, dones in seq:
        again.step(rew.to(gpu), dones.to(gpu).to(torch.uint8))    # (uint8 dones: the same kernel path)
    assert again._deques is None
    assert torch.equal(again.rings, st.rings) and torch.equal(again.count, st.count)
    assert torch.equal(again.cur_sum, st.cur_sum) and torch.equal(again.cur_len, st.cur_len)


def test_other_dtypes_take_the_torch_path(gpu):
    from legged_gym_amd.rl.episode_stats import EpisodeStats
    seq = random_sequence(num_envs=65, steps=6, p=0.2, all_done_step=4)
    st, ref = EpisodeStats(65, gpu, capacity=7), DequeStats(65, "cpu", capacity=7)
    for t, (rew, dones) in enumerate(seq):
        ref.step(rew, dones)
        # the first two steps on the kernel, then float dones: the ring's contents carry over
        st.step(rew.to(gpu), dones.to(gpu) if t < 2 else dones.to(gpu).float())
        st.request()
        assert st.result() == ref.lists(), t
    assert st._deques is not None and torch.equal(st.cur_sum.cpu(), ref.cur_reward_sum)


def test_bad_arguments_launch_nothing(gpu):
    from legged_gym_amd.rl.episode_stats import EpisodeStats
    from legged_gym_amd.sim import abi
    st = EpisodeStats(65, gpu)
    lib = st._lib
    rew, dones = torch.ones(65, device=gpu), torch.ones(65, dtype=torch.uint8, device=gpu)
    stream = C.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    good = [rew.data_ptr(), dones.data_ptr(), 65, st.cur_sum.data_ptr(), st.cur_len.data_ptr(),
            st.ring_sum.data_ptr(), st.ring_len.data_ptr(), 100, st.count.data_ptr(), stream]
    bad = [{i: None} for i in (0, 1, 3, 4, 5, 6, 8)]
    bad += [{2: 0}, {2: -1}, {7: 0}, {7: -5}, {7: abi.EPISODE_RING_MAX + 1}]
    for change in bad:
        args = list(good)
        for i, v in change.items():
            args[i] = v
        assert lib.lgx_episode_stats_step(*args) == -1, change       # LGX_EINVAL
        assert b"lgx_episode_stats_step" in lib.lgx_last_error()
    torch.cuda.synchronize()
    assert int(st.count.item()) == 0 and not st.cur_len.any() and not st.rings.any()
    with pytest.raises(ValueError):
        EpisodeStats(65, gpu, capacity=abi.EPISODE_RING_MAX + 1)
    assert lib.lgx_episode_stats_step(*good) == 0
    assert int(st.count.item()) == 65 and st.result() == ([1.0] * 65, [1.0] * 65)
