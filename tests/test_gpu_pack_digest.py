"""Every C weight packer writes the bits it wrote when tests/golden/pack_digests.json was recorded (tools/pack_digest.py: seeded weights, the
packer called directly into a NaN-filled buffer, SHA-256 of the input and of the packed bytes per case).  A packer bug is silent -- a wrong
word is a wrong weight, not a fault -- so the layouts are pinned word for word: plain, 16-bit, folded, split-half (all four forms), Linear,
F(2,3), F(4,3) on each slab form, the F(4,2) sub-pixel phases; padded shapes; scales 2^0 and 2^17."""
import json
import os

import pytest

from _tools import ROOT, load_script

pytestmark = pytest.mark.gpu

TOOL = load_script('tools/pack_digest.py')
with open(os.path.join(ROOT, 'tests', 'golden', 'pack_digests.json')) as fh:
    GOLD = json.load(fh)


def test_the_golden_file_holds_the_case_table():
    assert sorted(GOLD) == sorted(TOOL.CASES)


@pytest.mark.parametrize('name', sorted(TOOL.CASES))
def test_packed_bits_match_the_recorded_digest(name):
    src, packed = TOOL.digest(name)
    assert src == GOLD[name]['input'], f'{name}: the seeded weight differs from the recorded one (the RNG stream moved): not a packer failure'
    assert packed == GOLD[name]['packed'], f'{name}: {TOOL.CASES[name][1]} wrote other bits than recorded'
