"""CPU: the numpy model of a verification step under sampling and a repetition penalty (tests/qwen_lookup_sampling_model.py) against
hand-computed cases, and every named defect caught by the probe inputs the GPU tests run (tests/test_gpu_lm_pick_verify.py,
tests/test_gpu_lookup_step_mark.py, tests/test_gpu_qwen_lookup_sampling.py)."""
import numpy as np

import qwen_lookup_model as LM
import qwen_lookup_sampling_model as SM

MAP_DEFECTS = ("sees_own_draft", "misses_last_draft", "repeat_twice", "seen_and_draft_twice", "pick_writes_seen")
MARK_DEFECTS = ("marks_rejected", "own_token_unmarked")


def test_the_map_rule_on_hand_cases():
    seen = np.zeros(8, dtype=np.uint8)
    seen[2] = 1
    drafts = [4, 4, 2, 9, -3, 7]
    assert [np.flatnonzero(SM.penalised(8, seen, drafts, r)).tolist() for r in range(7)] == \
        [[2], [2, 4], [2, 4], [2, 4], [2, 4], [2, 4], [2, 4, 7]]                 # row r sees drafts 0..r-1; 9 and -3 are no ids of V = 8
    assert int(SM.penalised(8, seen, drafts, 6).max()) == 1                      # once, however often an id occurs
    assert SM.penalised(8, seen, [], 0).tolist() == seen.tolist()                # one row reads no draft


def test_the_penalty_is_transformers_rule_in_fp32():
    z = np.array([8.0, -8.0, 0.3, -0.3], dtype=np.float32)
    once = SM.penalise(z, np.array([1, 1, 1, 0]), 2.0)
    assert once.dtype == np.float32 and once.tolist() == [4.0, -16.0, np.float32(0.3) / np.float32(2.0), np.float32(-0.3)]
    assert SM.penalise(z, np.array([2, 2, 0, 0]), 2.0).tolist()[:2] == [2.0, -32.0]


def test_the_probe_holds_and_each_map_defect_breaks_it():
    assert SM.probe_holds()
    for d in MAP_DEFECTS:
        assert not SM.probe_holds(d), f"the probe does not catch {d!r}"
    z, seen, drafts, pen = SM.probe()
    assert z.shape == (9, 16) and len(drafts) == 8 and set(np.unique(z).tolist()) == {-8.0, 8.0} and pen == 2.0


def test_the_mark_cases_hold_and_each_mark_defect_breaks_one():
    for c in SM.MARK_CASES:
        assert SM.mark_case_holds(c), c[0]
    for d in MARK_DEFECTS:
        assert [c[0] for c in SM.MARK_CASES if not SM.mark_case_holds(c, d)], f"no case catches {d!r}"


def _runs():
    """(lm, prompt, uniforms, the plain run, T) for a few seeds: the inputs every replay below shares."""
    out = []
    for seed in range(6):
        lm = SM.toy_lm(12, seed)
        rng = np.random.default_rng(100 + seed)
        prompt, T = rng.integers(0, 12, 5).tolist(), 14
        u = rng.random(T)
        out.append((lm, prompt, u, SM.plain(lm, prompt, u, T), T))
    return out


def _guesses(G):
    wrong3 = [t if (i + 1) % 3 else (t + 1) % 12 for i, t in enumerate(G)]
    return (("all right", list(G)), ("every 3rd wrong", wrong3), ("all wrong", [(t + 1) % 12 for t in G]))


def test_a_replay_gives_the_plain_run_whatever_the_drafts_and_k():
    for lm, prompt, u, G, T in _runs():
        for K in (1, 3, 7, 31):
            for name, guess in _guesses(G):
                toks, stats = SM.replay(lm, prompt, u, guess, K, T)
                assert toks == G, (K, name)
                assert stats == LM.simulate_guess(G, guess, K, T), (K, name)     # the counts of the greedy loop's host simulation


def test_each_loop_defect_changes_a_replayed_run():
    for d in ("marks_rejected", "own_token_unmarked", "uniform_from_zero", "pick_writes_seen", "sees_own_draft", "misses_last_draft"):
        changed = 0
        for lm, prompt, u, G, T in _runs():
            for K in (3, 7):
                for name, guess in _guesses(G):
                    changed += SM.replay(lm, prompt, u, guess, K, T, d)[0] != G
        assert changed, f"no replay catches {d!r}"


def test_every_named_defect_is_covered_above():
    covered = set(MAP_DEFECTS) | set(MARK_DEFECTS) | {"uniform_from_zero"}
    assert covered == set(SM.DEFECTS) and len(SM.DEFECTS) == 8
