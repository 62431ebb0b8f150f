"""tests/launch_plan_driver.cpp behind a fixture, for tests/test_launch_plan.py and the tests that size launches of their own scenes."""
import pytest

import host_driver


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = host_driver.build(tmp_path_factory.mktemp("launch_plan"), "launch_plan", ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror"])

    def ask(*requests):
        return host_driver.ask(exe, *requests)
    ask.exe = exe
    return ask


def one(plan, cmd, **kw):
    return plan((cmd, kw))[0]
