"""``_CapturePolicy`` of the trainer - which training steps are captured into a HIP graph, which are replayed, and when data-parallel ranks
take their one vote on it - as a table of calls and answers.  Plain Python: the policy sees batch keys and "is this batch padded" only.
The data-parallel patterns are those ``test_gpu_ddp.py::test_capture_agreement_happens_at_a_fixed_call_on_every_rank`` runs on a process
group; a mistake in this rule is a hang there."""
import pytest

from cldrd_amd.trainer import nway_listwise as TL

P = TL._CapturePolicy
W = TL.NwayTrainer._DDP_WARM


def drive(policy, calls, capture_ok=lambda key: True):
    """What ``NwayTrainer._train_step_graph`` does with the answers: a VOTE_NO is a "no" in the agreement, a CAPTURE is tried and - under
    ``ddp`` - its outcome voted; either way the agreed outcome is recorded.  ``calls``: [(key, padded)].  -> answers, [(call number, vote)]"""
    answers, votes = [], []
    for key, padded in calls:
        a = policy.decide(key if padded else None, padded)
        if a == P.VOTE_NO:
            votes.append((policy.calls, False))
            policy.record(key, False)
        elif a == P.CAPTURE:
            ok = capture_ok(key)
            if policy.ddp:
                votes.append((policy.calls, ok))
            policy.record(key, ok)
        answers.append(a)
    return answers, votes


def padded_packed(pattern):
    """one padded shape "A"; True = this call's batch is packed (not eligible)"""
    return [("A", not packed) for packed in pattern]


def test_warm_up_count_is_three():
    assert W == 3


def test_ddp_all_padded_votes_yes_at_call_w_plus_1_and_replays():
    pol = P(W, ddp=True)
    answers, votes = drive(pol, padded_packed([False] * (W + 3)))
    assert votes == [(W + 1, True)]
    assert answers == [P.EAGER] * W + [P.CAPTURE, P.REPLAY, P.REPLAY] and not pol.broken


def test_ddp_packed_batch_at_the_agreement_call_votes_no():
    pol = P(W, ddp=True)
    answers, votes = drive(pol, padded_packed([False] * W + [True, False, False, True]))
    assert votes == [(W + 1, False)]
    assert answers == [P.EAGER] * W + [P.VOTE_NO] + [P.EAGER] * 3 and pol.broken and not pol.captured


def test_ddp_packed_batches_before_the_agreement_call_vote_no():
    pol = P(W, ddp=True)
    answers, votes = drive(pol, padded_packed([True, True, False, False, False, False]))
    assert votes == [(W + 1, False)]                          # (padded at call W + 1, but seen once, not W times)
    assert answers == [P.EAGER] * W + [P.VOTE_NO] + [P.EAGER] * 2 and pol.broken and not pol.captured


def test_ddp_always_packed_still_votes_at_the_same_call():
    pol = P(W, ddp=True)
    answers, votes = drive(pol, padded_packed([True] * (W + 2)))
    assert votes == [(W + 1, False)]
    assert answers == [P.EAGER] * W + [P.VOTE_NO, P.EAGER] and pol.broken


def test_ddp_eager_forever_after_a_no():
    pol = P(W, ddp=True)
    drive(pol, padded_packed([True] * (W + 1)))
    calls = pol.calls
    answers, votes = drive(pol, padded_packed([False] * 10))
    assert answers == [P.EAGER] * 10 and votes == [] and pol.calls == calls        # (nothing is counted any more either)


def test_ddp_two_shapes_before_the_agreement_call_vote_no():
    pol = P(W, ddp=True)
    answers, votes = drive(pol, [("A", True), ("B", True), ("A", True), ("A", True), ("A", True)])
    assert votes == [(W + 1, False)] and answers == [P.EAGER] * W + [P.VOTE_NO, P.EAGER]


def test_ddp_only_the_agreed_shape_replays_and_nothing_is_voted_on_again():
    pol = P(W, ddp=True)
    answers, votes = drive(pol, [("A", True)] * (W + 1) + [("B", True)] * (W + 2) + [("A", True), ("A", False), ("A", True)])
    assert votes == [(W + 1, True)]
    assert answers == [P.EAGER] * W + [P.CAPTURE] + [P.EAGER] * (W + 2) + [P.REPLAY, P.EAGER, P.REPLAY]
    assert pol.captured == {"A"} and pol.calls == 2 * W + 6


def test_ddp_a_capture_that_another_rank_lost_leaves_everything_eager():
    pol = P(W, ddp=True)
    answers, votes = drive(pol, padded_packed([False] * (W + 3)), capture_ok=lambda key: False)
    assert votes == [(W + 1, False)] and answers == [P.EAGER] * W + [P.CAPTURE, P.EAGER, P.EAGER] and pol.broken and not pol.captured


def test_one_gpu_one_shape_three_eager_calls_then_capture_then_replay():
    pol = P(W, ddp=False)
    answers, votes = drive(pol, [("A", True)] * 7)
    assert answers == [P.EAGER] * 3 + [P.CAPTURE] + [P.REPLAY] * 3 and votes == [] and pol.calls == 0


def test_one_gpu_packed_calls_do_not_count():
    pol = P(W, ddp=False)
    answers, _ = drive(pol, [("A", False), ("A", True), ("A", False), ("A", True), ("A", True), ("A", False), ("A", True), ("A", True)])
    assert answers == [P.EAGER] * 6 + [P.CAPTURE, P.REPLAY]


@pytest.mark.parametrize("order", ["round_robin", "fifth_arrives_late"])
def test_one_gpu_five_shapes_interleaved_capture_the_first_four_only(order):
    pol = P(W, ddp=False)
    if order == "round_robin":
        calls = [(k, True) for _ in range(6) for k in "ABCDE"]
    else:
        calls = [(k, True) for _ in range(2) for k in "ABCD"] + [(k, True) for _ in range(6) for k in "AEBECEDE"]
    answers, _ = drive(pol, calls)
    per_shape = {k: [a for (key, _), a in zip(calls, answers) if key == k] for k in "ABCDE"}
    for k in "ABCD":
        n = len(per_shape[k])
        assert per_shape[k] == [P.EAGER] * 3 + [P.CAPTURE] + [P.REPLAY] * (n - 4), k
    assert set(per_shape["E"]) == {P.EAGER} and pol.captured == set("ABCD") and "E" not in pol.seen


def test_one_gpu_a_failed_capture_leaves_everything_eager():
    pol = P(W, ddp=False)
    calls = [("A", True)] * 4 + [("B", True)] * 4 + [("A", True)] * 3 + [("C", True)] * 5
    answers, _ = drive(pol, calls, capture_ok=lambda key: key != "B")
    assert answers == [P.EAGER] * 3 + [P.CAPTURE] + [P.EAGER] * 3 + [P.CAPTURE] + [P.EAGER] * 8 and pol.broken
