------------------------------ MODULE lost ------------------------------
(* Written to show: <>Q STARTS AT THE INITIAL STATES, []<>Q ANYWHERE.  Q (q = 1) is true initially, lost by the one step of a fair process and never recurs.  <>(q = 1)  HOLDS: no initial state is a ~Q state.  []<>(q = 1)  is VIOLATED: the behaviour stutters for ever in the final state, where q = 0. *)
EXTENDS Naturals

(* --algorithm lost
variables q = 1;

fair process Lose = 0
begin
  L: q := 0;
end process

end algorithm *)

Once == <>(q = 1)
Again == []<>(q = 1)
=============================================================================
