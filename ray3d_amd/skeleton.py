"""Joint trees for the bone terms of the validation losses (evaluate.clip_valid, r3d_clip_valid_losses).

A tree is a sequence `parents` of J ints: parents[0] == -1 (the root) and 0 <= parents[j] < j for every other joint, so a
parent always comes before its children.  Bone j-1 is joint parents[j] minus joint j - for H36M_17_PARENTS the sixteen columns
of lib/skeleton/bone.py:51-68, in that order.
"""
from __future__ import annotations

from typing import Sequence, Tuple

MAX_JOINTS = 17

# the 17-joint Human3.6M skeleton of the reference (bone.py:51-68: 0-1, 1-2, 2-3, 0-4, 4-5, 5-6, 0-7, 7-8, 8-9, 9-10, 8-11, 11-12,
# 12-13, 8-14, 14-15, 15-16)
H36M_17_PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 9, 8, 11, 12, 8, 14, 15)
# bones (bone index = child joint - 1) that are mirror images of each other: right / left leg, left / right arm
H36M_17_BONE_PAIRS = ((0, 3), (1, 4), (2, 5), (10, 13), (11, 14), (12, 15))


def validate_parents(parents: Sequence[int], num_joints: int) -> Tuple[int, ...]:
    """The tree as a tuple of ints, or ValueError: the rules r3d_clip_valid_losses enforces, with the joint named."""
    tree = tuple(int(v) for v in parents)
    if not 1 <= num_joints <= MAX_JOINTS:
        raise ValueError("num_joints must be in 1..%d (got %d)" % (MAX_JOINTS, num_joints))
    if len(tree) != num_joints:
        raise ValueError("a parent table of %d entries for %d joints" % (len(tree), num_joints))
    if tree[0] != -1:
        raise ValueError("parents[0] must be -1, the root (got %d)" % tree[0])
    for j in range(1, num_joints):
        if not 0 <= tree[j] < j:
            raise ValueError("parents[%d] must be in 0..%d: a parent comes before its children (got %d)" % (j, j - 1, tree[j]))
    return tree
