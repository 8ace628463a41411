"""tests/scratchcheck.py on an MI355X: every call of the sequence gives back the scratch it took, and so do the calls that host
code refuses after an allocation (argument and capacity errors; nothing here provokes a device fault)."""
import pytest

import scratchcheck
from centroflye_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


def test_every_call_gives_back_what_it_took(engine, report):
    scratchcheck.check_balanced(engine, report)


def test_refusals_behind_an_allocation_give_it_back(engine, report):
    scratchcheck.check_refusals(engine, report)
