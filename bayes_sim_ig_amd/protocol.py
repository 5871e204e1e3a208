"""The chunk protocol of run_training (reference mdnn.py:206-211, :235) as pure host functions: the one
statement of it in the package (the tests keep restatements of their own, on purpose)."""


def split_rows(n_tot, test_frac):
    """(n_train, n_test) of a chunk of ``n_tot`` pairs: the last ``test_frac`` of it is held out, at least
    one pair trains (mdnn.py:206-211)."""
    n_train = max(int(n_tot * (1.0 - test_frac)), 1)
    return n_train, n_tot - n_train


def eval_updates(n_updates):
    """(every, [it, ...]): the held-out loss is logged at six points: every fifth of the updates and after
    the last (mdnn.py:235)."""
    every = max(n_updates // 5, 1)
    return every, [it for it in range(n_updates) if it % every == 0 or it + 1 == n_updates]
