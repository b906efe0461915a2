"""A deterministic automaton over token ids: what a TenantSession made with session(constraints=True) restricts a request's output to
(include/bitdelta_hip.h, bd_srv_constrain_rows, defines the mask; bd_srv_step_constrain_advance the transition).  Host integers only -- there
is no tokenizer and there are no strings here; a regex or schema compiler outside this project feeds from_edges."""
import operator


def _index(v, what):
    try:
        if isinstance(v, bool):
            raise TypeError
        return operator.index(v)
    except TypeError:
        raise ValueError("%s = %r: an integer is required" % (what, v))


class TokenAutomaton:
    """States 0 .. n_states - 1, the start state is 0.  The edges are kept in CSR form: the edges of state s are off[s] .. off[s + 1] - 1 of
    edge_tok / edge_next, sorted by token, no token twice within a state.  accepting[s] (0 / 1): in an accepting state the request's own stop
    ids are allowed next to the state's edges.  A state that is accepting and has no edges is FINAL: reaching it completes the constraint and
    retires the request (reason 8).  The attributes are plain lists of ints; an automaton is not modified after it is made.

    The constructors refuse (ValueError) what no request could use: a negative token, a state out of range, a token twice within a state, a state
    that is not accepting and has no edges (nothing would be allowed there).  What depends on the session and the request -- the vocabulary, the
    sizes the session holds, whether the request has stop ids -- is checked by `check`, which admission calls before it touches anything."""

    def __init__(self, n_states, off, edge_tok, edge_next, accepting):
        self.n_states, self.off, self.edge_tok, self.edge_next, self.accepting = n_states, off, edge_tok, edge_next, accepting

    # ------------------------------------------------------------ constructors
    @classmethod
    def from_edges(cls, n_states, edges, accepting):
        """The general form: n_states states, edges = triples (state, token, next_state) in any order, accepting = one truth value per state."""
        S = _index(n_states, "n_states")
        if S < 1:
            raise ValueError("n_states = %r: at least the start state is required" % (n_states,))
        accepting = [1 if a else 0 for a in accepting]
        if len(accepting) != S:
            raise ValueError("%d accepting flags for %d states" % (len(accepting), S))
        per = [[] for _ in range(S)]
        for tr in edges:
            try:
                s, y, nx = tr
            except (TypeError, ValueError):
                raise ValueError("an edge is a triple (state, token, next_state), not %r" % (tr,))
            s, y, nx = _index(s, "an edge's state"), _index(y, "an edge's token"), _index(nx, "an edge's next state")
            if not (0 <= s < S and 0 <= nx < S):
                raise ValueError("edge (%d, %d, %d): a state is outside 0 .. %d" % (s, y, nx, S - 1))
            if not (0 <= y < 1 << 31):
                raise ValueError("edge (%d, %d, %d): a token id is >= 0 (and fits 32 bits)" % (s, y, nx))
            per[s].append((y, nx))
        off, tok, nxt = [0], [], []
        for s in range(S):
            per[s].sort()
            for (a, _), (b, _) in zip(per[s], per[s][1:]):
                if a == b:
                    raise ValueError("state %d has two edges on token %d: the automaton is deterministic" % (s, a))
            if not per[s] and not accepting[s]:
                raise ValueError("state %d is not accepting and has no edges: nothing would be allowed there" % s)
            tok += [y for y, _ in per[s]]
            nxt += [nx for _, nx in per[s]]
            off.append(len(tok))
        return cls(S, off, tok, nxt, accepting)

    @classmethod
    def from_choices(cls, choices):
        """The trie of a list of non-empty token lists (vLLM's guided_choice on token ids): the output is exactly one of them.  The node that ends
        a choice is accepting; a choice that is a prefix of another ends in a node that is accepting and not final (the request's stop id ends
        it there, another token goes on).  Duplicates collapse.  Nodes are numbered in the order the choices create them, the root is 0."""
        choices = [[_index(y, "a token") for y in c] for c in choices]
        if not choices or any(not c for c in choices):
            raise ValueError("from_choices takes at least one choice, each of at least one token")
        children, accepting, edges = [{}], [0], []
        for c in choices:
            s = 0
            for y in c:
                if y not in children[s]:
                    children.append({})
                    accepting.append(0)
                    children[s][y] = len(children) - 1
                    edges.append((s, y, len(children) - 1))
                s = children[s][y]
            accepting[s] = 1
        return cls.from_edges(len(children), edges, accepting)

    @classmethod
    def allowed_set(cls, tokens):
        """The one-state automaton with a self-loop on every token of `tokens`, accepting (vLLM's allowed_token_ids): every output token lies in
        the set, and the request ends as it would otherwise -- its stop ids (allowed in addition), max_new_tokens, the cache."""
        toks = sorted(set(_index(y, "a token") for y in tokens))
        if not toks:
            raise ValueError("allowed_set takes at least one token")
        return cls.from_edges(1, [(0, y, 0) for y in toks], [1])

    # ------------------------------------------------------------ the rule on host integers
    @property
    def n_edges(self):
        return len(self.edge_tok)

    def edges(self, s):
        """state s's edges as a list of (token, next_state), sorted by token"""
        return list(zip(self.edge_tok[self.off[s]:self.off[s + 1]], self.edge_next[self.off[s]:self.off[s + 1]]))

    def is_final(self, s):
        return bool(self.accepting[s]) and self.off[s] == self.off[s + 1]

    def allowed(self, s, stop_ids=()):
        """the sorted token ids state s allows a request with these stop ids to emit"""
        a = set(self.edge_tok[self.off[s]:self.off[s + 1]])
        if self.accepting[s]:
            a |= set(int(i) for i in stop_ids if int(i) >= 0)
        return sorted(a)

    def step(self, s, token):
        """the state after `token` in state s: the edge's target, or s itself when the state has no edge on it (a stop id in an accepting state)"""
        for y, nx in self.edges(s):
            if y == token:
                return nx
        return s

    def check(self, vocab, max_states, max_edges, has_stop_ids):
        """What admission checks before anything is touched (ValueError): every token < vocab; no more states or edges than the session holds; and
        a start state that is accepting and has no edges needs a stop id, because nothing else could be the first token -- any OTHER such state
        is final and needs none, the request ends on reaching it."""
        if self.n_states > max_states or self.n_edges > max_edges:
            raise ValueError("the automaton has %d states and %d edges: this session holds %d and %d (session(max_constraint_states=, "
                             "max_constraint_edges=))" % (self.n_states, self.n_edges, max_states, max_edges))
        if self.edge_tok and max(self.edge_tok) >= vocab:
            raise ValueError("the automaton has an edge on token %d, outside the vocabulary of %d" % (max(self.edge_tok), vocab))
        if self.is_final(0) and not has_stop_ids:
            raise ValueError("the start state is accepting and has no edges, and the request has no stop ids: nothing would be allowed")
        return self
