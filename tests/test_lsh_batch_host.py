"""Host-side checks of the LSH batches: _run_key's matcher element, _multi_batch's routing of
LSH runs (synthesis functions stubbed), the IA_LSH_BATCH switch, and the two C-ABI entries'
binding and their refusals that need no device.  No device."""
import types

import pytest
import torch


def cfg(**kw):
    c = types.SimpleNamespace(num_ch=1, max_levels=3, matcher='brute', k=1.0, weights=[1.0] * 55,
                              convert=True, remap_lum=False, init_rand=True, AB_weight=1, n_sm=3, levels=None)
    for f, v in kw.items():
        setattr(c, f, v)
    return c


def pyrs(shapes=((5, 6), (10, 12), (20, 24)), fill=0.0):
    mk = lambda: [torch.full(s, fill, dtype=torch.float64) for s in shapes]  # noqa: E731
    return mk(), [mk()], mk(), mk()


def test_run_key_separates_matchers():
    import image_analogies as ia
    A, Ap, B, _ = pyrs()
    key = lambda c: ia._run_key(c, A, Ap, B)  # noqa: E731
    exact, lsh = cfg(), cfg(matcher='lsh')
    assert key(exact)[-1] is None
    assert key(lsh)[-1] is not None and key(lsh) != key(exact)
    hash(key(lsh))
    assert key(lsh) == key(cfg(matcher='lsh'))
    assert key(lsh) == key(cfg(matcher='lsh', lsh_tables=16, lsh_hashes=4, lsh_width=1.0, lsh_seed=0))
    for f, v in (('lsh_tables', 8), ('lsh_hashes', 3), ('lsh_width', 2.0), ('lsh_seed', 5)):
        assert key(cfg(matcher='lsh', **{f: v})) != key(lsh), f
        assert key(cfg(matcher='lsh', **{f: v})) == key(cfg(matcher='lsh', **{f: v})), f
    # the LSH settings of an exact run do not split exact runs
    assert key(cfg(lsh_tables=8)) == key(exact)
    # and the other elements still separate
    assert key(lsh) != ia._run_key(lsh, A, Ap + Ap, B)
    assert key(lsh) != key(cfg(matcher='lsh', max_levels=2))
    assert dict(key(cfg(matcher='lsh', lsh_tables=8))[-1]) == dict(tables=8, hashes=4, width=1.0, seed=0)


@pytest.fixture
def routed(monkeypatch, tmp_path):
    """_multi_batch with the setup, the synthesis functions and the outputs stubbed: yields
    (run maker, log of ('batch', job count, kappas, lsh) / ('one', kappa, lsh) calls)."""
    import _ia
    import image_analogies as ia
    log = []

    def batch(jobs, max_levels, ks, weights, debug=False, **kw):
        log.append(('batch', len(jobs), tuple(ks), kw.get('lsh'), 'lsh' in kw))
        return [{} for _ in jobs]

    def one(A, Ap, B, Bp, max_levels, k, weights, lsh=None, debug=False):
        log.append(('one', k, lsh))
        return {}
    monkeypatch.setattr(ia, 'synthesize_batch_dev', batch)
    monkeypatch.setattr(ia, 'synthesize_dev', one)
    monkeypatch.setattr(ia, 'setup_dev', lambda A, Aps, B, c: pyrs(fill=float(A)) + ([],))
    monkeypatch.setattr(ia, '_read', lambda f: int(f[1:]))
    monkeypatch.setattr(ia, 'save_metadata', lambda *a: None)
    monkeypatch.setattr(ia, 'write_outputs', lambda *a, **k: None)
    monkeypatch.setattr(_ia, 'to_dev', lambda w: torch.as_tensor(w))
    monkeypatch.setattr(torch.cuda, 'synchronize', lambda *a: None)
    monkeypatch.delenv('IA_LSH_BATCH', raising=False)
    monkeypatch.setitem(ia.LSH_BATCH_DEFAULT, False, 1)
    monkeypatch.setitem(ia.LSH_BATCH_DEFAULT, True, 1)

    def run(j, a, k, **over):
        return (j, ('A%d' % a, ['P%d' % a], 'B%d' % j, str(tmp_path / ('o%d' % j)) + '/', dict(over, k=k)))
    return run, log


LSH = dict(tables=16, hashes=4, width=1.0, seed=0)


def test_equal_lsh_runs_make_one_batch_call(routed):
    import image_analogies as ia
    run, log = routed
    out = ia._multi_batch([run(0, 1, 0.5), run(1, 1, 2.0), run(2, 2, 3.0)], cfg(matcher='lsh'), False)
    assert sorted(out) == [0, 1, 2]
    assert log == [('batch', 3, (0.5, 2.0, 3.0), LSH, True)]


def test_exact_runs_pass_no_lsh_keyword(routed):
    import image_analogies as ia
    run, log = routed
    ia._multi_batch([run(0, 1, 0.5), run(1, 1, 2.0)], cfg(), False)
    assert log == [('batch', 2, (0.5, 2.0), None, False)]


def test_mixed_runs_make_separate_calls(routed):
    import image_analogies as ia
    run, log = routed
    group = [run(0, 1, 0.5), run(1, 1, 1.5, matcher='brute'), run(2, 1, 2.5, lsh_tables=8),
             run(3, 1, 3.5), run(4, 1, 4.5, lsh_tables=8), run(5, 1, 5.5, matcher='brute'),
             run(6, 1, 6.5, lsh_seed=3)]
    ia._multi_batch(group, cfg(matcher='lsh'), False)
    assert log == [('batch', 2, (0.5, 3.5), LSH, True),
                   ('batch', 2, (1.5, 5.5), None, False),
                   ('batch', 2, (2.5, 4.5), dict(LSH, tables=8), True),
                   ('one', 6.5, dict(LSH, seed=3))]


def test_a_lone_lsh_run_goes_to_synthesize_dev(routed):
    import image_analogies as ia
    run, log = routed
    ia._multi_batch([run(0, 1, 0.5)], cfg(matcher='lsh'), False)
    assert log == [('one', 0.5, LSH)]


def test_switch_sends_lsh_runs_one_by_one(routed, monkeypatch):
    import image_analogies as ia
    run, log = routed
    group = [run(0, 1, 0.5), run(1, 1, 2.0)]
    monkeypatch.setenv('IA_LSH_BATCH', '0')
    ia._multi_batch(group, cfg(matcher='lsh'), False)
    assert log == [('one', 0.5, LSH), ('one', 2.0, LSH)]
    del log[:]
    ia._multi_batch(group, cfg(), False)                   # (exact runs do not look at it)
    assert log == [('batch', 2, (0.5, 2.0), None, False)]
    del log[:]
    # unset: the row type's default; set: it decides for both row types
    monkeypatch.delenv('IA_LSH_BATCH')
    monkeypatch.setitem(ia.LSH_BATCH_DEFAULT, False, 0)
    assert not ia.lsh_batch_enabled(False) and ia.lsh_batch_enabled(True)
    ia._multi_batch(group, cfg(matcher='lsh'), False)
    assert [e[0] for e in log] == ['one', 'one']
    monkeypatch.setenv('IA_LSH_BATCH', '1')
    assert ia.lsh_batch_enabled(False) and ia.lsh_batch_enabled(True)


def test_synthesize_jobs_passes_lsh_through(monkeypatch):
    import image_analogies as ia
    log = []
    monkeypatch.setattr(ia, 'synthesize_batch_dev',
                        lambda jobs, *a, **k: log.append(('batch', len(jobs), k.get('lsh'))) or [{}] * len(jobs))
    monkeypatch.setattr(ia, 'synthesize_dev', lambda *a, **k: log.append(('one', k.get('lsh'))) or {})
    jobs = [pyrs() for _ in range(3)]
    ia.synthesize_jobs(jobs, 3, 1.0, None, batch=2, lsh=LSH)
    assert log == [('batch', 2, LSH), ('one', LSH)]
    del log[:]
    ia.synthesize_jobs(jobs, 3, 1.0, None, batch=2)
    assert log == [('batch', 2, None), ('one', None)]


def test_entries_bound_and_refuse_without_a_device():
    import _ia
    new = {'ia_synth_levels_lsh_batch', 'ia_synth_levels3_lsh_batch'}
    assert new <= set(_ia.declared_symbols()) and new <= set(_ia._SIGS)
    lib = _ia.lib()
    arr = (_ia.IaSynthArgs * 129)()
    for name in sorted(new):
        fn = getattr(lib, name)
        for K in (0, 129, -1):
            assert fn(arr, 1, K, None) == _ia.IA_E_ARG, (name, K)
            msg = lib.ia_last_error().decode()
            assert msg.startswith(name) and 'K out of range' in msg, msg
        assert fn(None, 1, 2, None) == _ia.IA_E_ARG, name
        assert lib.ia_last_error().decode().startswith(name)
        assert fn(arr, 0, 2, None) == _ia.IA_E_ARG and fn(arr, 65, 2, None) == _ia.IA_E_ARG, name
        # a level without lsh is refused before anything is looked into
        assert fn(arr, 1, 2, None) == _ia.IA_E_ARG, name
        assert 'lsh' in lib.ia_last_error().decode()
