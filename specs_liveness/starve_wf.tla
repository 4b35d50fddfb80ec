------------------------------ MODULE starve_wf ------------------------------
(* A fair process waits for its turn while a fair process keeps flipping the turn: under WEAK fairness the waiter may starve, for it is disabled in every other state of the cycle.  (Once the waiter got through, everybody finishes.) *)
EXTENDS Naturals

(* --algorithm starve_wf
variables turn = 0, got = 0;

fair process Waiter = 0
begin
  W:   await turn = 1;
  Got: got := 1;
end process

fair process Flipper = 1
begin
  F: while got = 0 do
       turn := 1 - turn;
     end while;
end process

end algorithm *)
=============================================================================
