------------------------------ MODULE fairplus_plus ------------------------------
(* Written to show: `+` UNDER `fair+` MEANS NOTHING: the Waiter is `fair+` and its label `W:+` adds no conjunct (SF_vars(Waiter) covers it).  Termination HOLDS, and the whole report equals fairplus_plain's, the same algorithm without the `+`. *)
EXTENDS Naturals

(* --algorithm fairplus_plus
variables turn = 0, got = 0;

fair+ process Waiter = 0
begin
  W:+   await turn = 1;
  Got: got := 1;
end process

fair process Toggler = 1
begin
  F: while got = 0 do
       turn := 1 - turn;
     end while;
end process

end algorithm *)

=============================================================================
