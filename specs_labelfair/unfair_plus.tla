------------------------------ MODULE unfair_plus ------------------------------
(* Written to show: A LABEL MODIFIER IN AN UNFAIR PROCESS MEANS NOTHING: the Waiter is a plain `process`, its `W:+` adds no conjunct, and the fair Toggler may flip for ever.  Termination is VIOLATED.  Were the `+` honoured, SF_vars(W) would make the Waiter move and Termination would hold. *)
EXTENDS Naturals

(* --algorithm unfair_plus
variables turn = 0, got = 0;

process Waiter = 0
begin
  W:+  await turn = 1;
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
