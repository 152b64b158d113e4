"""CPU: `reflection_loop` / `best_index` of regione_amd/adapters/thinking.py against Step1XEditV1P2/inplace.py:192-212 and :470-543, with
a scripted thinker and a fake `edit_once`.  Every expected value is written out from the cited reference lines, none is computed by
the code under test."""
import pytest

from regione_amd.adapters.thinking import LoopResult, best_index, reflection_loop


class Scripted:
    """think -> "T(<prompt>)"; reflect -> the next (text, scores) of the script; format_text -> the next verdict.  Every call is logged."""

    def __init__(self, reflections=(), verdicts=()):
        self.reflections, self.verdicts, self.log = list(reflections), list(verdicts), []

    def think(self, image, prompt):
        self.log.append(("think", image, prompt))
        return f"T({prompt})"

    def reflect(self, ref_image, image, prompt):
        self.log.append(("reflect", ref_image, image, prompt))
        return self.reflections.pop(0)

    def format_text(self, text):
        self.log.append(("format_text", text))
        return self.verdicts.pop(0)


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the thinker is not touched with both switches off ({name})")


def info(s1, s2):
    return {"score1": {"score": list(s1)}, "score2": {"score": list(s2)}}


def editor():
    """edit_once(image, prompt) -> ["E<k>(image|prompt)"], k the try; `.calls` lists what it was handed."""
    calls = []

    def edit_once(image, prompt):
        calls.append((image, prompt))
        return [f"E{len(calls)}({image}|{prompt})"]
    edit_once.calls = calls
    return edit_once


def reflects(t):
    return [c for c in t.log if c[0] == "reflect"]


def test_success_on_the_first_try():
    t, e = Scripted([("ok <#Success>", info([4, 5], [3]))], [(True, None)]), editor()
    r = reflection_loop(e, t, "IMG", "make it red", False, True, 3)
    assert isinstance(r, LoopResult) and e.calls == [("IMG", "make it red")]                       # :212 ends on success
    assert r.images == ["E1(IMG|make it red)"] and r.final_images == ["E1(IMG|make it red)"]        # :473, :521
    assert r.think_info == ["ok <#Success>"] and r.best_info == [info([4, 5], [3])] and r.reformat_prompt is None and r.tries == 1
    assert t.log == [("reflect", "IMG", "E1(IMG|make it red)", "make it red"), ("format_text", "ok <#Success>")]    # no think (:199-200)


def test_a_failure_with_a_refine_prompt_edits_the_edited_image_with_it():
    t = Scripted([("worse", info([2], [2])), ("fine <#Success>", info([5], [5]))], [(False, "make it redder"), (True, None)])
    e = editor()
    r = reflection_loop(e, t, "IMG", "make it red", False, True, 3)
    first = "E1(IMG|make it red)"
    assert e.calls == [("IMG", "make it red"), (first, "make it redder")]                          # :477-479
    assert r.images == [first, f"E2({first}|make it redder)"] and r.tries == 2
    assert r.final_images == [r.images[1]]                                                         # 25 > 4 (:508)
    assert r.think_info == ["worse", "fine <#Success>"]
    # reflect always sees the ORIGINAL image and the prompt as it stood after thinking (:209-210, :471)
    assert [c[1:] for c in reflects(t)] == [("IMG", first, "make it red"), ("IMG", r.images[1], "make it red")]


def test_a_failure_without_one_goes_back_to_the_original_image_and_the_reformatted_prompt():
    t = Scripted([("bad", info([1], [1])), ("good <#Success>", info([1], [1]))], [(False, None), (True, None)])
    e = editor()
    r = reflection_loop(e, t, "IMG", "make it red", True, True, 3)
    assert t.log[0] == ("think", "IMG", "make it red") and r.reformat_prompt == "T(make it red)"   # :198
    assert e.calls == [("IMG", "T(make it red)"), ("IMG", "T(make it red)")]                       # :201, :481-482
    assert [c[1:] for c in reflects(t)] == [("IMG", r.images[0], "T(make it red)"), ("IMG", r.images[1], "T(make it red)")]
    assert r.final_images == [r.images[1]]                                                         # a tie: success beats none (:514)


def test_a_refined_try_that_fails_without_a_refine_prompt_returns_to_the_original():
    t = Scripted([("a", info([1], [1])), ("b", info([1], [1])), ("c", info([1], [1]))], [(False, "P2"), (False, None), (False, None)])
    e = editor()
    r = reflection_loop(e, t, "IMG", "P", True, True, 3)
    assert e.calls == [("IMG", "T(P)"), ("E1(IMG|T(P))", "P2"), ("IMG", "T(P)")]                   # :482 is reformat_prompt, not "P"
    assert all(c[1] == "IMG" and c[3] == "T(P)" for c in reflects(t)) and r.tries == 3


@pytest.mark.parametrize("max_try_cnt", [1, 2, 3])
def test_the_loop_gives_up_at_max_try_cnt(max_try_cnt):
    n = max_try_cnt
    t, e = Scripted([(f"no{i}", info([3 - i], [1])) for i in range(n)], [(False, None)] * n), editor()
    r = reflection_loop(e, t, "IMG", "P", False, True, max_try_cnt)
    assert len(e.calls) == n and r.tries == n and len(r.images) == len(r.think_info) == len(r.best_info) == n     # :212, :483
    assert r.final_images == [r.images[0]]                                                         # 3 > 2 > 1: the first try scored best


def test_max_try_cnt_defaults_to_three():
    t, e = Scripted([("no", info([1], [1]))] * 3, [(False, None)] * 3), editor()
    assert reflection_loop(e, t, "IMG", "P", False, True).tries == 3                               # :109


def test_thinking_alone_is_one_attempt_on_the_reformatted_prompt():
    t, e = Scripted(), editor()
    r = reflection_loop(e, t, "IMG", "P", True, False, 3)
    assert t.log == [("think", "IMG", "P")] and e.calls == [("IMG", "T(P)")]                       # :198, :201, :484-486
    assert r.images == ["E1(IMG|T(P))"] and r.final_images == ["E1(IMG|T(P))"]                     # out_images = image; :491
    assert r.think_info == [] and r.best_info == [] and r.reformat_prompt == "T(P)" and r.tries == 1     # :203-204 stay empty


def test_with_both_switches_off_it_is_one_attempt_and_no_thinker():
    e = editor()
    r = reflection_loop(e, Untouchable(), "IMG", "P", False, False, 5)                             # :205-206: max_try_cnt = 1
    assert e.calls == [("IMG", "P")] and r.images == ["E1(IMG|P)"] and r.final_images == ["E1(IMG|P)"]
    assert r.think_info is None and r.best_info is None and r.reformat_prompt is None and r.tries == 1
    r = reflection_loop(editor(), None, "IMG", "P", None, None)                                    # unspecified is off
    assert r.images == ["E1(IMG|P)"]


# ---- best-of selection (:496-521) ------------------------------------------------------------------------------------------------------
def test_a_strictly_larger_score_wins_whatever_the_success_marks():
    # scores 2*3 = 6, 4*2 = 8, 7*1 = 7 (the MIN of each list): entry 1, although only entry 0 carries the mark
    assert best_index(["<#Success>", "", ""], [info([2, 9], [3]), info([4, 6], [2, 5]), info([7], [1, 8])]) == 1
    assert best_index(["", ""], [info([3], [3]), info([2], [4])]) == 0                             # 9 > 8: a later, smaller one does not win
    assert best_index([""], [info([0], [0])]) == 0                                                 # 0 > -1 (:497)


def test_on_a_tie_a_success_beats_an_entry_without_it():
    assert best_index(["", "x <#Success> y", ""], [info([2], [2])] * 3) == 1                       # :514-516; the third does not retake it
    assert best_index(["<#Success>", ""], [info([2], [2])] * 2) == 0                               # neither :514 nor :518 fires


def test_on_a_tie_with_equal_success_status_the_later_entry_wins():
    assert best_index(["", "", ""], [info([2], [2])] * 3) == 2                                     # :518-519
    assert best_index(["<#Success>", "<#Success>"], [info([1, 5], [4])] * 2) == 1
    assert best_index(["<#Success>", "", "<#Success>"], [info([2], [2])] * 3) == 2


def test_a_missing_thinking_text_counts_as_no_success():
    assert best_index(["<#Success>"], [info([1], [1]), info([1], [1])]) == 0                       # :505: "" for the entry without text


def test_final_images_follow_the_selection_in_the_loop():
    t = Scripted([("a <#Success>", info([3], [2])), ("b", info([2], [3])), ("c", info([1], [1]))],
                 [(False, None), (False, None), (False, None)])
    r = reflection_loop(editor(), t, "IMG", "P", False, True, 3)
    assert r.final_images == [r.images[0]]                                                         # 6 == 6: the marked entry keeps it


def test_no_try_at_all_leaves_everything_empty():
    r = reflection_loop(editor(), Scripted(), "IMG", "P", False, True, 0)
    assert r.images == [] and r.final_images == [] and r.think_info == [] and r.tries == 0         # :212 never enters; :491
