"""tools/isa_same.py: the comparison of two {kernel: (body hash, lines)} tables, on hand-made tables (no compiler involved)."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "isa_same", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "isa_same.py"))
isa_same = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_same)

A, B, C = ("aaaa", 10), ("bbbb", 20), ("cccc", 30)


def test_without_the_option_a_rename_is_a_loss():
    rows, ok = isa_same.compare({"kept": A, "old_name": B}, {"kept": A, "new_name": B})
    assert rows == [("SAME", "kept"), ("only in old", "old_name"), ("only in new", "new_name")] and not ok


def test_renamed_and_identical():
    rows, ok = isa_same.compare({"kept": A, "old_name": B}, {"kept": A, "new_name": B}, renamed=True)
    assert rows == [("SAME", "kept"), ("SAME (renamed)", "old_name -> new_name")] and ok


def test_renamed_and_different():
    rows, ok = isa_same.compare({"kept": A, "old_name": B}, {"kept": A, "new_name": C}, renamed=True)
    assert rows == [("SAME", "kept"), ("only in old", "old_name"), ("only in new", "new_name")] and not ok


def test_a_missing_kernel_and_a_changed_one():
    rows, ok = isa_same.compare({"kept": A, "gone": B}, {"kept": C, "added": A}, renamed=True)
    assert rows == [("only in old", "gone"), ("DIFFERENT", "kept"), ("only in new", "added")] and not ok
    rows, ok = isa_same.compare({"kept": A}, {"kept": A, "added": B}, renamed=True)
    assert rows == [("SAME", "kept"), ("only in new", "added")] and ok


def test_two_old_kernels_with_equal_bodies_pair_one_to_one():
    rows, ok = isa_same.compare({"old_1": B, "old_2": B}, {"new_1": B}, renamed=True)
    assert rows == [("SAME (renamed)", "old_1 -> new_1"), ("only in old", "old_2")] and not ok
    rows, ok = isa_same.compare({"old_1": B, "old_2": B}, {"new_1": B, "new_2": B}, renamed=True)
    assert rows == [("SAME (renamed)", "old_1 -> new_1"), ("SAME (renamed)", "old_2 -> new_2")] and ok


def test_the_name_filter_applies_to_either_side():
    rows, ok = isa_same.compare({"conv_old": B, "other": A}, {"conv_new": B, "other": C}, "conv", renamed=True)
    assert rows == [("SAME (renamed)", "conv_old -> conv_new")] and ok
