"""The CPU oracle at state rounds 16..31 and at the exact ties of the median
rule, for every scenario tests/test_gpu_state_edges.py replays on the GPU.

For each scenario (tests/state_edges.py) and every round, every cell of every
online node: the oracle's next state equals a plain restatement of
MessageState::next_round (src/message_state.rs:86-171) applied to the dumped
state, record summary and |peers_in_this_round|.  Then the coverage the
scenario exists for is asserted from the same dumps -- B rounds and
rounds_in_state_b up to max_rounds - 1 (bit 4 of the 5-bit field set), the
exits by the round limit from B and from C, the vote grid -- so the GPU tests,
which replay the same inputs on every engine layout, cannot go vacuous.
"""
import pytest

import state_edges as se
from state_edges import CODE_D, CODE_NEW_B, TAG_B, TAG_C, Coverage, next_code


def _b(rnd, our):
    return (TAG_B << 14) | (our << 7) | rnd


def _c(rib, rnd):
    return (TAG_C << 14) | (rnd << 7) | rib


def test_restatement_by_hand():
    p = (3, 3, 32)
    assert next_code(CODE_NEW_B, 0, 0, p) == _b(1, 1)           # nobody heard: ge = less = 0
    assert next_code(_b(30, 1), 0, 5, p) == _b(31, 1)
    assert next_code(_b(31, 1), 0x8000 | 3, 3, p) == CODE_D      # the limit comes before the votes
    assert next_code(_b(30, 2), 0x8000, 1, p) == _c(31, 0)       # a peer in C
    assert next_code(_b(15, 1), 20, 40, p) == _b(16, 1)          # 2 ge = |P|: strict
    assert next_code(_b(15, 1), 21, 40, p) == _b(16, 2)
    assert next_code(_b(15, 2), (20 << 7) | 40, 40, p) == _b(16, 2)   # counter-1 copies vote "less" at 2
    assert next_code(_b(15, 2), (21 << 7) | 21, 41, p) == _c(16, 0)
    assert next_code(_c(31, 0), 0, 0, p) == CODE_D               # 1 + 31 >= 32
    assert next_code(_c(30, 0), 0, 0, p) == _c(30, 1)
    assert next_code(_c(30, 1), 0, 0, p) == CODE_D
    assert next_code(_c(29, 2), 0, 0, p) == CODE_D               # by rib and by max_c_rounds alike
    assert next_code(_c(28, 1), 0, 0, p) == _c(28, 2)
    assert next_code(_c(28, 2), 0, 0, p) == CODE_D               # by max_c_rounds
    assert next_code(_b(15, 1), 0, 3, (3, 3, 16)) == CODE_D
    assert next_code(_b(15, 1), 0, 3, (3, 3, 17)) == _b(16, 1)
    assert next_code(_b(4, 1), 1, 1, (2, 2, 32)) == _c(5, 0)     # counter_max 2
    assert next_code(CODE_D, 0, 9, p) == CODE_D


@pytest.mark.parametrize("name,schedule", [(k, "2P") for k in sorted(se.STAGGERED)] +
                         [(k, "SEQ") for k in se.SEQ_TOO])
def test_staggered(oracle, name, schedule):
    n, R, params, faults = se.STAGGERED[name]
    cov = Coverage()
    rounds = se.run_staggered(n, R, params, faults, schedule, cov=cov)
    assert 7 <= rounds <= 90 and cov.cells >= 7 * n * R * (1 - 2 * faults[0])
    se.staggered_conditions(cov, params)


@pytest.mark.parametrize("R,schedule", [(64, "2P"), (64, "SEQ"), (32, "2P"), (16, "2P")])
def test_vote_grid(oracle, R, schedule):
    cov = Coverage(votes=True)
    se.run_votes(R, schedule=schedule, cov=cov)
    se.vote_conditions(cov, R)
    assert cov.c_by_counter and cov.c_to_d_maxc > 0   # the majorities took the cells on to C and D


@pytest.mark.parametrize("R,schedule", [(64, "2P"), (64, "SEQ"), (16, "2P")])
def test_lifetimes(oracle, R, schedule):
    # folded onto 16 columns the 64 scripts run in four node groups: every
    # rib stays covered, so the conditions are the same
    cov = Coverage()
    se.run_lifetimes(R, schedule=schedule, cov=cov)
    se.lifetime_conditions(cov)
